"""Classification on the GPU (cirkit_amd/classification.py, cirkit_amd/csrc/ck_class.hip): the class head against its fp64
restatement, `HipClassifierTrainer`'s gradients against fp64 autograd through the oracle, its optimizer step, the bad-label
policy, unit padding, `HipClassifier`'s predictions (with missing features), `HipCircuitModule` over a K-unit root, shards."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from class_head_restatement import class_head, uniform_log_prior

REL = 1e-4  # tests/test_gpu_parity.py

PLANS = {
    "qg4_k3_c3": dict(shape=(1, 4, 4), region_graph="quad-graph", sum_product_layer="cp", input_layer="categorical", K=3, C=3),
    "qt8_k8_c10": dict(shape=(1, 8, 8), region_graph="quad-tree-2", sum_product_layer="cp", input_layer="categorical", K=8, C=10),
    "qt8_k32_c10": dict(shape=(1, 8, 8), region_graph="quad-tree-2", sum_product_layer="cp", input_layer="categorical", K=32, C=10),
    "pd4_gauss_k4_c5": dict(shape=(1, 4, 4), region_graph="poon-domingos", sum_product_layer="cp", input_layer="gaussian", K=4, C=5),
    "qt4_tucker_k4_c70": dict(shape=(1, 4, 4), region_graph="quad-tree-2", sum_product_layer="tucker", input_layer="categorical", K=4, C=70),
}
OBJECTIVES = [(1.0, 0.0), (0.0, 1.0), (0.3, 1.0)]


@functools.lru_cache(maxsize=None)
def _case(name, B=70):
    """(plan, tensors, x, y) of a plan of the table: init_plan_tensors(seed=3), data from Generator(5), every 7th row unlabelled."""
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.templates import image_data

    p = PLANS[name]
    plan = image_data(p["shape"], p["region_graph"], input_layer=p["input_layer"], num_input_units=p["K"],
                      sum_product_layer=p["sum_product_layer"], num_sum_units=p["K"], num_classes=p["C"])
    tensors = init_plan_tensors(plan, seed=3)
    g = torch.Generator().manual_seed(5)
    D = int(np.prod(p["shape"]))
    x = torch.randn(B, D, generator=g) if p["input_layer"] == "gaussian" else torch.randint(0, 256, (B, D), generator=g)
    y = torch.randint(0, p["C"], (B,), generator=g)
    y[::7] = -1
    return plan, tensors, x, y


def _objective(out, y, pi, w, gB):
    """The loss of the contract in torch, on the oracle's (B, 1, C) output: returns (L, sum gen, sum disc, mean |j_y|)."""
    j = out[:, 0, :] + pi.to(out.dtype)
    e = torch.logsumexp(j, dim=1)
    lab = y >= 0
    jy = j.gather(1, y.clamp(min=0)[:, None])[:, 0]
    gen = torch.where(lab, jy, e)
    disc = torch.where(lab, jy - e, torch.zeros_like(e))
    return -(w[0] * gen.sum() + w[1] * disc.sum()) / gB, gen.sum().detach(), disc.sum().detach(), jy[lab].abs().mean().detach()


def _oracle(plan, tensors, x, y, w, dtype, gB=None):
    from oracle.torch_oracle import as_torch, evaluate_plan

    C = _num_classes(plan)
    tt = {k: v.clone().to(dtype).requires_grad_(True) for k, v in as_torch(tensors).items()}  # (never the cached arrays)
    if dtype == torch.float64:
        torch.set_default_dtype(torch.float64)
    try:
        out = evaluate_plan(plan, tt, x, grad=True)
        L, gen, disc, jy = _objective(out, y, torch.from_numpy(uniform_log_prior(C)), w, float(gB or x.shape[0]))
        L.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return {k: v.grad for k, v in tt.items()}, float(L.detach()), float(gen), float(disc), float(jy), out.detach()


@functools.lru_cache(maxsize=None)
def _oracle_cached(name, w):
    plan, tensors, x, y = _case(name)
    return _oracle(plan, tensors, x, y, w, torch.float64), _oracle(plan, tensors, x, y, w, torch.float32)


def _num_classes(plan):
    from cirkit_amd.classification import num_classes

    return num_classes(plan)


def _check_grads(got, ref, ref32, names, what=""):
    """The bounds of tests/test_training.py::test_hip_backward_matches_autograd, tensor by tensor."""
    noisy = []
    for k in names:
        g, want = got[k].double(), ref[k]
        scale = float(want.abs().max())
        err = float((g - want).abs().max())
        err32 = float((ref32[k].double() - want).abs().max())
        print(f"{what} {k}: scale {scale:.3e} err {err:.3e} err32 {err32:.3e}")
        if err32 > 0.05 * scale:
            noisy.append(k)
            assert err <= 50.0 * err32, (k, err, err32, scale)
            r32 = float(ref32[k].double().reshape(-1, want.shape[-1]).sum(-1).abs().max())
            assert float(g.reshape(-1, g.shape[-1]).sum(-1).abs().max()) <= 8.0 * r32 + 16.0 * err32, (k, r32, err32)
            continue
        assert err <= 5e-4 * scale + 6.0 * err32 + 1e-12, (k, err, err32, scale)
        n32 = abs(float(ref32[k].double().norm()) - float(want.norm()))
        assert abs(float(g.norm()) - float(want.norm())) <= 1e-3 * float(want.norm()) + 6.0 * n32 + 1e-12, k
    assert len(noisy) <= 0.35 * len(names), (noisy, len(names))


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------
def _ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def _block(B, C, stride, seed):
    rng = np.random.default_rng(seed)
    l = (rng.uniform(-50.0, 0.0, (B, C)) + rng.choice([-3000.0, -300.0, 0.0], (B, 1))).astype(np.float32)
    y = rng.integers(0, C, B).astype(np.int64)
    y[::7] = -1
    raw = rng.normal(size=C)
    if C > 2:
        raw[1] = -np.inf  # an impossible class
    pi = (raw - np.log(np.exp(raw[np.isfinite(raw)]).sum())).astype(np.float32)
    if C > 1:
        l[rng.random((B, C)) < 0.1] = -np.inf
    special = {}
    if B > 6:
        l[3, :] = -np.inf
        l[5, C // 2] = np.nan
        y[6] = C - 1
        l[6, C - 1] = -np.inf
        special = {"all_inf": 3, "nan": 5, "target_inf": 6}
    block = np.full((B, stride), 7.0, dtype=np.float32)  # (padded columns hold values nobody may read)
    block[:, :C] = l
    return block, l, y, pi, special


def _run_head(dev, block, C, y, pi, w, gB):
    from cirkit_amd.classification import ClassHead

    B, stride = block.shape
    head = ClassHead(C, pi, dev)
    xb = torch.from_numpy(block).to(dev)
    out = dict(seed=torch.full((B, stride), 9.0, device=dev), log_post=torch.empty((B, C), device=dev),
               log_evid=torch.empty(B, device=dev), pred=torch.empty(B, dtype=torch.int64, device=dev))
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    head.run(xb, labels=torch.from_numpy(y).to(dev), w_gen=w[0], w_disc=w[1], inv_gb=1.0 / gB, stats=True, bad_flag=flag, **out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, head.stats.cpu().numpy().copy(), int(flag.item())


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 2, 3, 10, 64, 65, 100])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_class_head_matches_restatement(hip_device, B, C):
    """Seed per entry within (|w_gen| + |w_disc|) / gB x (4 ulp32(max_c |j_bc|) + 4 x 2^-23): the exponent's argument comes
    from one fp32 sum and one fp32 difference of magnitude |j|, plus the exp's own few ulp.  Zero entries and dead rows
    exactly 0; predictions exact where the two best posteriors differ by more than that bound; counts exact, sums within
    1e-6 x sum |terms|; two calls bit-identical."""
    w, gB = (0.3, 1.0), float(B + 3)
    for stride in sorted({C, (C + 31) // 32 * 32}):
        block, l, y, pi, special = _block(B, C, stride, seed=1000 * B + C)
        want = class_head(l, y, pi, w[0], w[1], global_batch=gB)
        got, stats, flag = _run_head(hip_device, block, C, y, pi, w, gB)
        assert flag == 0
        jf = np.where(np.isfinite(want.joint), np.abs(want.joint), 0.0).max(axis=1)
        bound = (4.0 * _ulp32(jf) + 4.0 * 2.0 ** -23)[:, None]
        seed = got["seed"].astype(np.float64)
        assert np.isfinite(seed).all()
        err = np.abs(seed[:, :C] - want.seed) / ((abs(w[0]) + abs(w[1])) / gB)
        print(f"B {B} C {C} stride {stride}: seed err / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
        assert not seed[:, C:].any() and not seed[:, :C][want.seed == 0.0].any() and not seed[want.dead].any()
        for r in special.values():
            assert want.dead[r]
        ok = np.isfinite(want.log_evid)
        assert np.isnan(got["log_post"][~ok]).all() and (got["pred"][~ok] == -1).all()
        assert np.array_equal(np.isneginf(got["log_evid"]), np.isneginf(want.log_evid)) and np.array_equal(np.isnan(got["log_evid"]), np.isnan(want.log_evid))
        assert (np.abs(got["log_evid"][ok] - want.log_evid[ok]) <= 2.0 * _ulp32(want.log_evid[ok])).all()
        q, qw = got["log_post"][ok].astype(np.float64), want.log_post[ok]
        fin = np.isfinite(qw)
        assert np.array_equal(np.isneginf(q), np.isneginf(qw))
        assert (np.abs(q[fin] - qw[fin]) <= np.broadcast_to(bound[ok], qw.shape)[fin] * np.maximum(1.0, np.abs(qw[fin]))).all()
        if C > 1:  # predictions: exact where the two best differ by more than the bound
            top = np.sort(np.where(np.isnan(qw), -np.inf, qw), axis=1)
            with np.errstate(invalid="ignore"):
                clear = (top[:, -1] - top[:, -2]) > bound[ok][:, 0]
            assert (got["pred"][ok][clear] == want.pred[ok][clear]).all()
        else:
            assert (got["pred"][ok] == 0).all()
        assert np.array_equal(stats[2:], want.stats[2:])
        assert abs(stats[0] - want.stats[0]) <= 1e-6 * np.abs(want.gen).sum()
        assert abs(stats[1] - want.stats[1]) <= 1e-6 * np.abs(want.disc).sum()
        got2, stats2, _ = _run_head(hip_device, block, C, y, pi, w, gB)
        assert stats2.tobytes() == stats.tobytes() and got2["seed"].tobytes() == got["seed"].tobytes()


@pytest.mark.gpu
def test_class_head_flags_a_bad_label_and_serves_unlabelled_batches(hip_device):
    from cirkit_amd.classification import ClassHead

    block, l, y, pi, _ = _block(65, 10, 32, seed=4)
    for bad in (10, -2):
        yb = y.copy()
        yb[40] = bad
        want = class_head(l, yb, pi, 1.0, 1.0)
        got, stats, flag = _run_head(hip_device, block, 10, yb, pi, (1.0, 1.0), 65.0)
        assert flag == 1 and want.bad and want.dead[40] and not got["seed"][40].any()
        assert np.array_equal(stats[2:], want.stats[2:])
    # no labels at all (prediction only), uniform prior: every live row is unlabelled
    head = ClassHead(10, None, hip_device)
    post = torch.empty((65, 10), device=hip_device)
    head.run(torch.from_numpy(block).to(hip_device), log_post=post, stats=True)
    want = class_head(l, None, None)
    assert np.array_equal(head.stats.cpu().numpy()[2:], want.stats[2:]) and want.stats[3] == 0
    ok = np.isfinite(want.log_evid)
    q, qw = post.cpu().numpy()[ok].astype(np.float64), want.log_post[ok]
    fin = np.isfinite(qw)
    jf = np.where(np.isfinite(want.joint), np.abs(want.joint), 0.0).max(axis=1)
    bound = np.broadcast_to((4.0 * _ulp32(jf) + 4.0 * 2.0 ** -23)[ok][:, None], qw.shape)  # (the bound of the shape test)
    assert np.array_equal(np.isneginf(q), np.isneginf(qw))
    assert (np.abs(q[fin] - qw[fin]) <= bound[fin] * np.maximum(1.0, np.abs(qw[fin]))).all()


# ---- 2. gradients end to end ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w", OBJECTIVES)
@pytest.mark.parametrize("name", list(PLANS))
def test_classifier_gradients_match_autograd(hip_device, name, w):
    """`HipClassifierTrainer.loss_and_grads` against fp64 autograd through the oracle of the same loss, the yardstick the
    oracle's fp32 autograd; bounds and structure of tests/test_training.py::test_hip_backward_matches_autograd (second pass
    checked).  Losses: |sum gen / live - want| <= 1e-5 |want|; |sum disc / labelled - want| <= 2e-5 mean |j_y| (a difference
    of two quantities each held to the existing bound)."""
    from cirkit_amd.classification import HipClassifierTrainer

    plan, tensors, x, y = _case(name)
    (ref, L64, gen64, disc64, jy, _), (ref32, *_rest) = _oracle_cached(name, w)
    tr = HipClassifierTrainer(plan, tensors, device=hip_device, optimizer="sgd", generative_weight=w[0], discriminative_weight=w[1])
    assert not tr.fused and tr._jobs is None and tr.num_classes == PLANS[name]["C"]
    tr.loss_and_grads(x.to(hip_device), y.to(hip_device))
    st = tr.loss_and_grads(x.to(hip_device), y.to(hip_device)).cpu().numpy()
    torch.cuda.synchronize()
    B, lab = x.shape[0], int((y >= 0).sum())
    assert st[2] == B and st[3] == lab and st[5] == 0
    print(f"{name} {w}: gen {st[0] / B:.6f} want {gen64 / B:.6f}; disc {st[1] / lab:.6f} want {disc64 / lab:.6f}; mean|j_y| {jy:.3f}")
    assert abs(st[0] / B - gen64 / B) <= 1e-5 * abs(gen64 / B)
    assert abs(st[1] / lab - disc64 / lab) <= 2e-5 * jy
    _check_grads({k: tr.grads[k].cpu() for k in plan.tensors}, ref, ref32, list(plan.tensors), f"{name} {w}")


# ---- 3. the optimizer step ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sgd_step_is_parameters_minus_lr_times_gradients(hip_device):
    from cirkit_amd.classification import HipClassifierTrainer

    plan, tensors, x, y = _case("qt8_k8_c10")
    tr = HipClassifierTrainer(plan, tensors, device=hip_device, optimizer="sgd", lr=0.1, generative_weight=0.3)
    xd, yd = x.to(hip_device), y.to(hip_device)
    tr.loss_and_grads(xd, yd)
    before, grads = tr.parameters(), tr.gradients()
    tr.step(xd, yd)
    after = tr.parameters()
    for k in plan.tensors:
        want = before[k].astype(np.float64) - 0.1 * grads[k].astype(np.float64)
        assert np.abs(after[k] - want).max() <= 1e-6 * np.abs(want).max(), k
        assert np.abs(after[k] - before[k]).max() > 0
    assert tr.skipped_steps == 0


def _adam_losses_oracle(plan, tensors, x, y, w, dtype, steps, lr):
    from oracle.torch_oracle import as_torch, evaluate_plan

    tt = {k: v.clone().to(dtype).requires_grad_(True) for k, v in as_torch(tensors).items()}  # (never the cached arrays)
    opt = torch.optim.Adam(list(tt.values()), lr=lr)
    pi = torch.from_numpy(uniform_log_prior(_num_classes(plan)))
    losses = []
    if dtype == torch.float64:
        torch.set_default_dtype(torch.float64)
    try:
        for _ in range(steps):
            opt.zero_grad()
            L = _objective(evaluate_plan(plan, tt, x, grad=True), y, pi, w, float(x.shape[0]))[0]
            L.backward()
            opt.step()
            losses.append(float(L.detach()))
    finally:
        torch.set_default_dtype(torch.float32)
    return np.asarray(losses)


@pytest.mark.gpu
def test_adam_trajectory_matches_the_oracle_loop(hip_device):
    """Ten Adam steps (lr 0.05) on a fixed 64-row batch of the K = 8, C = 10 plan, default objective (cross-entropy), against
    torch.optim.Adam in fp64 over the oracle.  The bound on the loss trajectory is four times the deviation of the SAME loop
    with the oracle in fp32 from the fp64 one, measured here on the CPU in every run (`dev32`; on losses of 1.94 .. 1.69 it was 1.5e-5 on one host and
    9.9e-6 on another when this test was written: it depends on the host's ATen kernels) -- not a constant chosen in advance."""
    from cirkit_amd.classification import HipClassifierTrainer

    plan, tensors, x, y = _case("qt8_k8_c10")
    x, y = x[:64], y[:64]
    w, steps, lr = (0.0, 1.0), 10, 0.05
    l64 = _adam_losses_oracle(plan, tensors, x, y, w, torch.float64, steps, lr)
    l32 = _adam_losses_oracle(plan, tensors, x, y, w, torch.float32, steps, lr)
    dev32 = float(np.abs(l32 - l64).max())
    tr = HipClassifierTrainer(plan, tensors, device=hip_device, optimizer="adam", lr=lr)
    xd, yd = x.to(hip_device), y.to(hip_device)
    got = []
    for _ in range(steps):
        st = tr.step(xd, yd).cpu().numpy()
        got.append(-(w[0] * st[0] + w[1] * st[1]) / 64.0)
    dev = float(np.abs(np.asarray(got) - l64).max())
    print(f"adam trajectory: fp64 {l64[0]:.6f} -> {l64[-1]:.6f}; dev32 {dev32:.3e}; gpu dev {dev:.3e}; gpu {np.asarray(got)}; fp64 {l64}")
    assert l64[-1] < l64[0]
    assert dev <= 4.0 * dev32, (dev, dev32)


# ---- 4. a bad label -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_bad_label_step_changes_nothing(hip_device, optimizer):
    from cirkit_amd.classification import HipClassifierTrainer

    plan, tensors, x, y = _case("qt8_k8_c10")
    tr = HipClassifierTrainer(plan, tensors, device=hip_device, optimizer=optimizer, lr=0.05)
    xd, yd = x.to(hip_device), y.to(hip_device)
    tr.step(xd, yd)  # (moments that are not zero)
    tr.check_inputs()
    state = lambda: [t.clone() for t in (tr._flat_param, tr._m1, tr._m2) if t is not None]  # noqa: E731
    before, skipped = state(), tr.skipped_steps
    yb = yd.clone()
    yb[9] = 10
    tr.step(xd, yb)
    torch.cuda.synchronize()
    for a, b in zip(before, state()):
        assert torch.equal(a, b)
    if optimizer == "adam":  # (the counter is `ck_adam_step`'s: an SGD step is skipped the same way without being counted)
        assert tr.skipped_steps == skipped + 1
    else:
        assert tr.skipped_steps == skipped
    with pytest.raises(IndexError):
        tr.check_inputs()
    tr.check_inputs()  # reported once
    st = tr.step(xd, yd).cpu().numpy()  # the next clean step works
    assert st[2] == 70 and st[5] == 0 and np.isfinite(st[:2]).all()
    assert not torch.equal(before[0], tr._flat_param)
    tr.check_inputs()


# ---- 5. padded units ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_padded_trainer_matches_unpadded(hip_device):
    from cirkit_amd.classification import HipClassifierTrainer

    name, w = "qt8_k8_c10", (0.3, 1.0)
    plan, tensors, x, y = _case(name)
    (ref, *_a), (ref32, *_b) = _oracle_cached(name, w)
    tr = HipClassifierTrainer(plan, tensors, device=hip_device, optimizer="sgd", generative_weight=w[0], discriminative_weight=w[1],
                              pad_units=True)
    assert tr._pad_info is not None and tr.circuit.layers[int(tr.circuit._out_pairs[0, 0])].num_output_units == 32
    xd, yd = x.to(hip_device), y.to(hip_device)
    tr.loss_and_grads(xd, yd)
    st = tr.loss_and_grads(xd, yd).cpu().numpy()
    got = {k: torch.from_numpy(v) for k, v in tr.gradients().items()}
    assert all(tuple(got[k].shape) == tuple(plan.tensors[k][0]) for k in plan.tensors)
    _check_grads(got, ref, ref32, list(plan.tensors), "padded")
    plain = HipClassifierTrainer(plan, tensors, device=hip_device, optimizer="sgd", generative_weight=w[0], discriminative_weight=w[1])
    st0 = plain.loss_and_grads(xd, yd).cpu().numpy()
    assert np.array_equal(st[2:], st0[2:]) and np.abs(st[:2] - st0[:2]).max() <= 1e-5 * np.abs(st0[:2]).max()
    # the padded classes (copies of real units in the arena) get probability 0: the posterior over the 10 real ones sums to 1
    clf = tr.classifier()
    lp = clf.predict_log_proba(xd)
    assert tuple(lp.shape) == (70, 10)
    assert float((lp.double().exp().sum(1) - 1.0).abs().max()) <= 1e-5
    assert float((lp - plain.classifier().predict_log_proba(xd)).abs().max()) <= REL * float(lp.abs().max()) + 1e-4


# ---- 6. prediction --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_classifier_predictions_match_oracle(hip_device):
    """`HipClassifier` on the fused forward (K = 32, C = 10, 70 rows) against the restatement applied to the oracle's output:
    full evidence, a (D,) mask, a per-row (B, D) mask and sentinel entries (expected values as tests/test_marginals.py
    obtains them: the oracle's integrate_mask)."""
    from cirkit_amd.classification import HipClassifier
    from oracle.torch_oracle import as_torch, evaluate_plan

    plan, tensors, x, y = _case("qt8_k32_c10")
    prior = np.log(np.arange(1.0, 11.0))
    clf = HipClassifier(plan, tensors, device=hip_device, log_prior=prior)
    pi = prior - np.log(np.exp(prior).sum())
    g = torch.Generator().manual_seed(11)
    D = x.shape[1]
    m1 = torch.rand(D, generator=g) < 0.3
    mB = torch.rand(70, D, generator=g) < 0.3
    xs = torch.where(mB, torch.full_like(x, -1), x)
    xd = x.to(hip_device)
    for what, xin, mask_arg, mask_oracle in (("full", xd, None, None), ("mask (D,)", xd, m1.to(hip_device), m1[None, :].expand(70, D)),
                                             ("mask (B, D)", xd, mB.to(hip_device), mB), ("sentinels", xs.to(hip_device), None, mB)):
        out = evaluate_plan(plan, as_torch(tensors), x, integrate_mask=None if mask_oracle is None else mask_oracle.contiguous())
        l = out[:, 0, :].numpy()
        want = class_head(l, y.numpy(), pi.astype(np.float32))
        tol = REL * float(np.abs(l).max())
        ll = clf.class_log_likelihoods(xin, mask_arg).cpu().numpy()
        lp = clf.predict_log_proba(xin, mask_arg).cpu().numpy()
        ev = clf.log_evidence(xin, mask_arg).cpu().numpy()
        pr = clf.predict(xin, mask_arg).cpu().numpy()
        print(f"{what}: |ll| {np.abs(ll - l).max():.3e} |log_post| {np.abs(lp - want.log_post).max():.3e} "
              f"|evidence| {np.abs(ev - want.log_evid).max():.3e} tol {tol:.3e}")
        assert ll.shape == (70, 10) and np.abs(ll - l).max() <= tol
        assert np.abs(lp - want.log_post).max() <= tol and np.abs(ev - want.log_evid).max() <= tol
        top = np.sort(want.log_post, axis=1)
        clear = top[:, -1] - top[:, -2] > 2 * tol
        assert (pr[clear] == want.pred[clear]).all() and (pr == lp.argmax(1)).all()
    st = clf.score(xd, y.to(hip_device)).cpu().numpy()
    l = evaluate_plan(plan, as_torch(tensors), x)[:, 0, :].numpy()
    want = class_head(l, y.numpy(), pi.astype(np.float32))
    tol = REL * float(np.abs(l).max())
    top = np.sort(want.log_post, axis=1)
    unclear = int((top[:, -1] - top[:, -2] <= 2 * tol).sum())
    assert np.array_equal(st[2:4], want.stats[2:4]) and st[5] == 0 and abs(st[4] - want.stats[4]) <= unclear
    assert abs(st[0] - want.stats[0]) <= 70 * tol and abs(st[1] - want.stats[1]) <= 70 * 2 * tol
    clf.check_score_labels()


@pytest.mark.gpu
def test_trainers_classifier_sees_updates(hip_device):
    from cirkit_amd.classification import HipClassifierTrainer

    plan, tensors, x, y = _case("qt8_k8_c10")
    tr = HipClassifierTrainer(plan, tensors, device=hip_device, optimizer="sgd", lr=0.5)
    clf = tr.classifier()
    xd, yd = x.to(hip_device), y.to(hip_device)
    before = clf.predict_log_proba(xd).clone()
    s0 = clf.score(xd, yd).cpu().numpy()
    for _ in range(3):
        tr.step(xd, yd)
    after = clf.predict_log_proba(xd)
    s1 = clf.score(xd, yd).cpu().numpy()
    assert float((after - before).abs().max()) > 0.0
    assert s1[1] > s0[1]  # three SGD steps on the cross-entropy raise sum log p(y | x)
    st = tr.loss_and_grads(xd, yd).cpu().numpy()  # ... and it is what the trainer's own forward now computes
    assert abs(st[1] - s1[1]) <= 1e-4 * abs(s1[1])


# ---- 7. HipCircuitModule over a K-unit root --------------------------------------------------------------------------
@pytest.mark.gpu
def test_module_cross_entropy_matches_classifier_trainer(hip_device):
    """The notebook's loop: ``F.cross_entropy(m(x)[:, 0, :], y).backward()`` against
    `HipClassifierTrainer(generative_weight=0, discriminative_weight=1)` on a fully labelled batch: the same kernels, the seed
    once from torch's fp32 cross-entropy and once from the head.  The two seeds differ by fp32 rounding, which the cancelling
    discriminative gradient amplifies: measured gap 4.0e-9 on the input layer's gradient of scale 4.2e-5 (1e-4 of the scale,
    not the 1e-5 first hoped for), so both are held to the bound of
    test_classifier_gradients_match_autograd against fp64 autograd through the oracle, and to its leading term against each
    other."""
    from cirkit_amd.classification import HipClassifierTrainer
    from cirkit_amd.training import HipCircuitModule

    plan, tensors, x, y = _case("qt8_k8_c10")
    y = y.clone()
    y[::7] = 3  # fully labelled
    xd, yd = x.to(hip_device), y.to(hip_device)
    m = HipCircuitModule(plan, tensors, device=hip_device)
    out = m(xd)
    assert tuple(out.shape) == (70, 1, 10)
    loss = F.cross_entropy(out[:, 0, :], yd)
    loss.backward()
    tr = HipClassifierTrainer(plan, tensors, device=hip_device, optimizer="sgd")
    st = tr.loss_and_grads(xd, yd).cpu().numpy()
    assert abs(float(loss.detach()) + st[1] / 70.0) <= 1e-5 * abs(float(loss.detach()))
    ref, ref32 = (_oracle(plan, tensors, x, y, (0.0, 1.0), dt)[0] for dt in (torch.float64, torch.float32))
    _check_grads({k: p.grad.cpu() for k, p in m.named_tensors().items()}, ref, ref32, list(plan.tensors), "module")
    _check_grads({k: tr.grads[k].cpu() for k in plan.tensors}, ref, ref32, list(plan.tensors), "trainer")
    for k, p in m.named_tensors().items():
        want = tr.grads[k]
        gap = float((p.grad - want).abs().max())
        print(f"module vs trainer {k}: gap {gap:.3e} scale {float(want.abs().max()):.3e}")
        assert gap <= 5e-4 * float(want.abs().max()), k


# ---- 8. shards ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_shards_sum_to_the_full_batch(hip_device):
    from cirkit_amd.classification import HipClassifierTrainer

    name, w = "qt8_k8_c10", (0.3, 1.0)
    plan, tensors, x, y = _case(name)
    (ref, *_a), (ref32, *_b) = _oracle_cached(name, w)
    tr = HipClassifierTrainer(plan, tensors, device=hip_device, optimizer="sgd", generative_weight=w[0], discriminative_weight=w[1])
    xd, yd = x.to(hip_device), y.to(hip_device)
    parts, stats = [], []
    for a, b in ((0, 35), (35, 70)):
        stats.append(tr.loss_and_grads(xd[a:b], yd[a:b], global_batch=70).cpu().numpy().copy())
        parts.append({k: tr.grads[k].cpu().clone() for k in plan.tensors})
    full = tr.loss_and_grads(xd, yd).cpu().numpy()
    total = stats[0] + stats[1]
    assert np.array_equal(total[2:], full[2:]) and np.abs(total[:2] - full[:2]).max() <= 1e-9 * np.abs(full[:2]).max()
    summed = {k: parts[0][k] + parts[1][k] for k in plan.tensors}
    _check_grads(summed, ref, ref32, list(plan.tensors), "shards")
    for k in plan.tensors:  # ... and against the full batch directly (fp32 sums in another order): the bound's leading term
        assert float((summed[k] - tr.grads[k].cpu()).abs().max()) <= 5e-4 * float(tr.grads[k].abs().max()), k
