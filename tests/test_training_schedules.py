"""The trainers driven through SCHEDULES of calls -- several batch sizes, explicit global batches, evicted and rebuilt bindings,
inference forwards between steps -- every call checked against fp64 autograd through the oracle.

What a real training loop does and a single-batch test never sees: a ragged last batch, evaluation forwards at other sizes,
gradient accumulation and uneven shards passing `global_batch`.  The trainers keep per-batch-size state (four sizes resident,
the oldest evicted) and recorded launch lists replayed by the native executor or as hipGraphs; a replay must point at the
buffers and constants of ITS key.  Every visit to a size brings a new batch: a replay that read a stale staging copy of an
earlier batch would be right on a reused one.  The staging copies of every binding a call evicts are kept alive here, so a
list that still points at them reads the old batch instead of memory the allocator may have handed on."""
import numpy as np
import pytest
import torch

from conftest import load_case
from test_training import _oracle_grads
from test_training_jobs import NOISY_TENSORS_ALLOWED, _case as _jobs_case


def _schedule(m, part=None):
    """(batch size, global batch) calls, "infer" (a forward of the circuit at a size no step uses) and "victim" (a step at the
    size that forward evicted from the circuit's bindings).  m: the largest size; part: one of the three sequences alone."""
    parts = {
        # eager, eager / recorded, replayed; then another global batch at the same size, and back (c's seed, -2 / gB)
        "global_batch": [(64, None)] * 3 + [(64, 128), (64, None)],
        # the same global batch at another size, and back (Z's seed, B / gB: Z has one binding, B = 1, for every size)
        "sizes": [(64, 128)] * 3 + [(33, 128), (64, 128)],
        # five sizes: 64 evicted, then rebuilt; a forward between two steps evicts a binding the next step needs
        "evictions": [(64, None)] * 3 + [(33, None), (17, None), (31, None), (m, None), (64, None), (1, None), "infer", "victim", (33, None)],
    }
    return parts[part] if part else [s for p in parts.values() for s in p]


def _visits(schedule):
    """The schedule with a batch seed per call: a new one whenever the size changes."""
    out, seed, last = [], 100, None
    for s in schedule:
        if isinstance(s, tuple) and s[0] != last:
            seed += 1
            last = s[0]
        out.append((s, seed))
    return out


def _hold_evicted(tr, B: int, held: list, arenas: dict) -> None:
    """Keep alive the staging copies of whatever state a call at batch size B evicts -- a launch list that still points at them
    then reads their old batch, deterministically wrong -- and set its arena aside for the state that is rebuilt at its size."""
    c = tr.circuit
    if B not in c._bindings and len(c._bindings) >= 4:
        bd = c._bindings[next(iter(c._bindings))]
        held += [t for t in (bd.xt, bd.xt_i) if t is not None]
        arenas[("circuit", bd.B)] = bd.arena
    sc = getattr(tr, "_signed", None)
    if sc is not None and B not in sc._bound and len(sc._bound) >= 4:
        B0 = next(iter(sc._bound))
        st = sc._bound[B0]
        held += [st.xt] + ([st.leaf.x64] if st.leaf is not None else [])
        arenas[("signed", B0)] = st.arena


def _same_arena_back(tr, B: int, arenas: dict, monkeypatch) -> None:
    """What torch's caching allocator usually does, made certain: the state rebuilt at size B gets the arena of the one evicted
    there, at the same address (the first allocation of its size and type in the call: `HipCircuit._bind`'s `torch.empty`,
    `_SignedCircuit.bind`'s `torch.zeros`).  A launch list judged valid by that address alone then replays over the other,
    moved buffers of the new state."""
    want = {}
    if B not in tr.circuit._bindings and ("circuit", B) in arenas:
        want["empty"] = arenas.pop(("circuit", B))
    sc = getattr(tr, "_signed", None)
    if sc is not None and B not in sc._bound and ("signed", B) in arenas:
        want["zeros"] = arenas.pop(("signed", B))
    for fn, old in want.items():
        real = getattr(torch, fn)

        def alloc(*a, _real=real, _old=old, _fn=fn, **k):
            if len(a) == 1 and a[0] == _old.numel() and k.get("dtype") == _old.dtype:
                monkeypatch.setattr(torch, _fn, _real)  # (once)
                return _old.zero_() if _fn == "zeros" else _old
            return _real(*a, **k)

        monkeypatch.setattr(torch, fn, alloc)


def _drive(tr, schedule, batch, check, monkeypatch, step=False):
    """Run the schedule on trainer `tr`; `check(where, ll, B, gB, x)` after every call."""
    dev = tr.device
    held: list = []
    arenas: dict = {}
    victim = None
    for i, (s, seed) in enumerate(_visits(schedule)):
        if s == "infer":
            c = tr.circuit
            victim = next(iter(c._bindings)) if len(c._bindings) >= 4 else 17
            _hold_evicted(tr, 45, held, arenas)
            y = c(batch(45, 7).to(dev))
            assert bool(torch.isfinite(y.real if y.is_complex() else y).all())
            continue
        B, gB = (victim, None) if s == "victim" else s
        x = batch(B, seed)
        _hold_evicted(tr, B, held, arenas)
        with monkeypatch.context() as mp:
            _same_arena_back(tr, B, arenas, mp)
            run = tr.step if step else tr.loss_and_grads
            ll = run(x.to(dev), global_batch=gB).clone()
        torch.cuda.synchronize()
        check(f"call {i}: B={B} global_batch={gB}", ll, B, float(B if gB is None else gB), x)


# ---- real circuits: HipTrainer --------------------------------------------------------------------------------------------------
_ORACLE: dict = {}


def _sum_grads(name, plan, tensors, x):
    """fp64 and fp32 autograd of -(1 / B) sum_b log p(x_b) and the fp64 loss, once per batch (the schedules of several trainers
    visit the same batches)."""
    k = (name, x.numpy().tobytes())
    if k not in _ORACLE:
        loss64, g64 = _oracle_grads(plan, tensors, x, torch.float64)
        _, g32 = _oracle_grads(plan, tensors, x, torch.float32)
        _ORACLE[k] = (loss64, g64, g32)
    return _ORACLE[k]


def _check_real(plan, got, want, want32, where):
    """`test_training.test_hip_backward_matches_autograd`'s bounds, on gradients of -(1 / gB) sum_b log p(x_b)."""
    noisy = []
    for k in plan.tensors:
        g = got[k].detach().cpu().double()
        scale = float(want[k].abs().max())
        err = float((g - want[k]).abs().max())
        err32 = float((want32[k] - want[k]).abs().max())
        if err32 > 0.05 * scale:  # (cancelling softmax gradients: the noise of the reference's fp32 autograd is the yardstick)
            noisy.append(k)
            assert err <= 50.0 * err32, (where, k, err, err32, scale)
            r32 = float(want32[k].reshape(-1, want[k].shape[-1]).sum(-1).abs().max())
            assert float(g.reshape(-1, g.shape[-1]).sum(-1).abs().max()) <= 8.0 * r32 + 16.0 * err32, (where, k, r32, err32)
            continue
        assert err <= 5e-4 * scale + 6.0 * err32 + 1e-12, (where, k, err, err32, scale)
        n32 = abs(float(want32[k].norm()) - float(want[k].norm()))
        assert abs(float(g.norm()) - float(want[k].norm())) <= 1e-3 * float(want[k].norm()) + 6.0 * n32 + 1e-12, (where, k)
    assert len(noisy) <= 0.35 * len(plan.tensors), (where, noisy, len(plan.tensors))


def _real_batch(g):
    xg = g["x"]
    if xg.dtype.kind == "f":
        return lambda B, seed: torch.randn((B, xg.shape[1]), generator=torch.Generator().manual_seed(seed))
    n = int(xg.max()) + 1
    return lambda B, seed: torch.randint(0, n, (B, xg.shape[1]), generator=torch.Generator().manual_seed(seed))


@pytest.mark.gpu
@pytest.mark.parametrize("name,fused", [("cfg1_rbt8", False), ("pd_gauss_6x6_k4", False), ("cfg2_qt784", True)])
def test_trainer_gradients_through_a_schedule_of_batch_sizes(hip_device, name, fused, monkeypatch):
    """Layer-wise and fused `HipTrainer` (the fused one at <= 100 rows: the fp64 oracle of 784 variables is the slow part)."""
    from cirkit_amd.training import HipTrainer

    plan, tensors, g = load_case(name)
    batch = _real_batch(g)
    tr = HipTrainer(plan, tensors, device=hip_device, optimizer="sgd", fused=fused, jobs=False)
    assert tr.fused == fused and tr._jobs is None

    def check(where, ll, B, gB, x):
        loss64, g64, g32 = _sum_grads(name, plan, tensors, x)
        assert float(ll[1]) == B and abs(float(ll[0]) + B * loss64) <= 1e-5 * abs(B * loss64), (where, float(ll[0]), -B * loss64)
        s = B / gB  # (the oracle's gradients are of -(1 / B) sum_b log p)
        _check_real(plan, tr.grads, {k: s * v for k, v in g64.items()}, {k: s * v.double() for k, v in g32.items()}, where)

    _drive(tr, _schedule(100), batch, check, monkeypatch)


@pytest.mark.gpu
def test_job_trainer_gradients_through_a_schedule_of_batch_sizes(hip_device, monkeypatch):
    """The job form (one recorded launch list per batch size; 8x8 QuadGraph, Categorical, CP, K = 64) beside the layer-wise
    trainer on the same schedule, with `test_training_jobs`' bounds.  Its lists read the circuit binding's staging copy of the
    batch and write its [sum, count] pair: after the inference forward evicts that binding, the next step at its size must
    not replay a list of the old one."""
    from cirkit_amd.training import HipTrainer

    plan, tensors, _ = _jobs_case("quadgraph_cat", 1)
    a = HipTrainer(plan, tensors, device=hip_device, optimizer="sgd", jobs=False)
    b = HipTrainer(plan, tensors, device=hip_device, optimizer="sgd", jobs=True)
    assert a._jobs is None and b._jobs is not None

    def batch(B, seed):
        return torch.randint(0, 256, (B, 64), generator=torch.Generator().manual_seed(seed))

    def check(where, lb, B, gB, x):
        la = a.loss_and_grads(x.to(hip_device), global_batch=int(gB)).clone()
        torch.cuda.synchronize()
        assert float(la[1]) == float(lb[1]) == B and abs(float(la[0] - lb[0])) <= 2e-6 * abs(float(la[0])), (where, float(la[0]), float(lb[0]))
        loss64, g64, g32 = _sum_grads("quadgraph_cat", plan, tensors, x)
        assert abs(float(lb[0]) + B * loss64) <= 1e-5 * abs(B * loss64), (where, float(lb[0]), -B * loss64)
        s = B / gB
        noisy = []
        for k in plan.tensors:
            ga, gb, want = a.grads[k].cpu().double(), b.grads[k].cpu().double(), s * g64[k]
            scale = float(want.abs().max()) + 1e-12
            err_a, err_b = float((ga - want).abs().max()), float((gb - want).abs().max())
            err32 = float((s * g32[k].double() - want).abs().max())
            if max(err32, err_a) > 0.05 * scale:
                noisy.append(k)
                assert err_b <= 50.0 * max(err32, err_a), (where, k, err_b, err_a, err32, scale)
                asum_b = float(gb.reshape(-1, gb.shape[-1]).sum(-1).abs().max())
                asum_a = float(ga.reshape(-1, ga.shape[-1]).sum(-1).abs().max())
                assert asum_b <= 4.0 * asum_a + 16.0 * max(err32, err_a), (where, k, asum_b, asum_a, err32, err_a)
                continue
            assert err_b <= 2.0 * err_a + 6.0 * err32 + 5e-4 * scale, (where, k, err_b, err_a, err32, scale)
            na = abs(float(ga.norm()) - float(want.norm()))
            assert abs(float(gb.norm()) - float(want.norm())) <= 2e-3 * float(want.norm()) + 2.0 * na + 1e-9, (where, k)
        assert len(noisy) <= NOISY_TENSORS_ALLOWED["quadgraph_cat"] * len(plan.tensors), (where, noisy, len(plan.tensors))

    _drive(b, _schedule(150), batch, check, monkeypatch)


# ---- squared circuits: HipSquaredTrainer ----------------------------------------------------------------------------------------
def _cfg5():
    import os

    from conftest import GOLDEN
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.plan import Plan

    plan_c, plan_z = Plan.load(os.path.join(GOLDEN, "cfg5_sos_c_k32")), Plan.load(os.path.join(GOLDEN, "cfg5_sos_z_k32"))
    # (the counter-based generator emits a few exact zeros: log 0 under autograd is NaN in the reference as well)
    tensors = {k: np.where(v == 0, np.float32(1e-2), v).astype(np.float32) for k, v in init_plan_tensors(plan_c).items()}
    return plan_c, plan_z, tensors


def _sq_batch(B, seed):
    return torch.randint(0, 256, (B, 784), generator=torch.Generator().manual_seed(seed))


def _sq_oracle(plan_c, plan_z, params, x, dtype=torch.float64):
    """Autograd through the oracle: (sum_b 2 Re c(x_b), its gradient, Re Z, its gradient) at `params` (fp64 results)."""
    from oracle import torch_oracle as oracle

    leaves = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).requires_grad_(True) for k, v in params.items()}
    if dtype == torch.float64:
        torch.set_default_dtype(torch.float64)
    try:
        c = (2.0 * oracle.evaluate_plan(plan_c, leaves, x, grad=True).real).sum()
        gc = torch.autograd.grad(c, list(leaves.values()))
        z = oracle.evaluate_plan(plan_z, leaves, None, grad=True).real.sum()
        gz = torch.autograd.grad(z, list(leaves.values()))
    finally:
        torch.set_default_dtype(torch.float32)
    return float(c), {k: g.double() for k, g in zip(leaves, gc)}, float(z), {k: g.double() for k, g in zip(leaves, gz)}


def _sq_grad(o, B, gB):
    """The gradient of -(1 / gB) sum_b 2 Re c(x_b) + (B / gB) Re Z from `_sq_oracle`'s parts."""
    _, gc, _, gz = o
    return {k: (-gc[k] / gB + (B / gB) * gz[k]).numpy() for k in gc}


def _sq_bound(want, want32):
    """`test_squared_trainer_on_baseline_config_5_against_the_oracles_autograd`'s bound, plus -- as the real circuits' checks
    have it -- six times the error of the reference's own fp32 autograd: at other batches than that test's the fp32 rounding
    of this circuit's gradients alone reaches 0.25 .. 0.75 % of their largest entry (measured on the host)."""
    return 2e-3 * max(1e-6, float(np.abs(want).max())) + 6.0 * float(np.abs(want32 - want).max())


_SQ_ORACLE: dict = {}


@pytest.mark.gpu
@pytest.mark.parametrize("part", ["global_batch", "sizes", "evictions"])
@pytest.mark.parametrize("signed,use_graph", [(False, False), (True, True), ("layers", False)])
def test_squared_trainer_gradients_through_a_schedule_of_batch_sizes(hip_device, signed, use_graph, part, monkeypatch):
    """c on the complex layer-wise lists, on signed-log blocks with the leaf region (replayed as hipGraphs) and on signed-log
    layers (`CK_SLSE_LEAF=0`).  The gradients are those of ``-(1 / gB) sum_b 2 Re c(x_b) + (B / gB) Re Z``: the seeds of c's
    and of Z's backward (-2 / gB, B / gB) differ between keys that share a binding, and every replayed list must carry its own."""
    from cirkit_amd.training_squared import HipSquaredTrainer

    if signed == "layers":
        monkeypatch.setenv("CK_SLSE_LEAF", "0")
        signed = True
    plan_c, plan_z, tensors = _cfg5()
    tr = HipSquaredTrainer(plan_c, tensors, plan_z=plan_z, device=hip_device, signed=signed, use_graph=use_graph, optimizer="sgd")
    assert (tr._signed is not None) == signed

    def check(where, ll, B, gB, x):
        key = x.numpy().tobytes()
        if key not in _SQ_ORACLE:
            _SQ_ORACLE[key] = (_sq_oracle(plan_c, plan_z, tensors, x), _sq_oracle(plan_c, plan_z, tensors, x, torch.float32))
        o64, o32 = _SQ_ORACLE[key]
        want_ll = o64[0] - B * o64[2]
        assert float(ll[1]) == B and abs(float(ll[0]) - want_ll) <= 1e-4 * abs(want_ll), (where, float(ll[0]), want_ll)
        got, want, want32 = tr.gradients(), _sq_grad(o64, B, gB), _sq_grad(o32, B, gB)
        for k in tensors:
            err = float(np.abs(got[k] - want[k]).max())
            assert err <= _sq_bound(want[k], want32[k]), (where, k, err, float(np.abs(want[k]).max()))

    _drive(tr, _schedule(50, part), _sq_batch, check, monkeypatch)


# ---- optimizer steps against an fp64 SGD replay ---------------------------------------------------------------------------------
_STEPS = [(33, 64), (64, 128), (64, 128), (64, 128), (17, 40)]  # (a key called three times before: recorded, then replayed)


def _close_to_replay(got, start, ref, where):
    """`test_squared_trainer_data_parallel_equals_single_process`' bound: a fraction of how far the parameter moved, plus two
    ulps of its magnitude."""
    for k in ref:
        moved = float(np.abs(ref[k] - start[k]).max())
        assert moved > 0.0, (where, k)
        ulp = 1.2e-7 * max(1.0, float(np.abs(ref[k]).max()))
        err = float(np.abs(got[k] - ref[k]).max())
        assert err <= 2e-3 * moved + 2 * ulp, (where, k, err, moved)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["layerwise", "fused", "jobs"])
def test_trainer_sgd_steps_through_a_schedule_match_an_fp64_replay(hip_device, path, monkeypatch):
    """`step()` at ragged sizes with explicit global batches -- layer-wise (the optimizer launch), fused (the optimizer in the
    backward epilogues), job mode 2 (the optimizer in the job epilogues) -- against SGD in fp64 driven by the oracle's
    gradients."""
    from cirkit_amd.training import HipTrainer

    lr = 0.05
    if path == "jobs":
        plan, tensors, _ = _jobs_case("quadgraph_cat", 1)

        def batch(B, seed):
            return torch.randint(0, 256, (B, 64), generator=torch.Generator().manual_seed(seed))
    else:
        plan, tensors, g = load_case("cfg1_rbt8" if path == "layerwise" else "cfg2_qt784")
        batch = _real_batch(g)
    tr = HipTrainer(plan, tensors, device=hip_device, optimizer="sgd", lr=lr, fused=path == "fused", jobs=path == "jobs")
    assert tr.fused == (path == "fused") and (tr._jobs is not None) == (path == "jobs")
    ref = {k: np.asarray(v, dtype=np.float64) for k, v in tensors.items()}
    start = {k: v.copy() for k, v in ref.items()}

    def check(where, ll, B, gB, x):
        loss64, g64 = _oracle_grads(plan, ref, x, torch.float64)  # (at the replay's parameters before this step)
        assert abs(float(ll[0]) + B * loss64) <= 1e-5 * abs(B * loss64), (where, float(ll[0]), -B * loss64)
        for k in ref:
            ref[k] -= lr * (B / gB) * g64[k].numpy()

    _drive(tr, _STEPS, batch, check, monkeypatch, step=True)
    _close_to_replay(tr.parameters(), start, ref, path)


@pytest.mark.gpu
def test_squared_trainer_sgd_steps_through_a_schedule_match_an_fp64_replay(hip_device, monkeypatch):
    """The squared trainer with the optimizer inside its recorded "end" list, at ragged sizes with explicit global batches.  Step
    by step from the trainer's own parameters: over several steps the fp32 rounding of the Embedding weights' gradients moves
    whole trajectories apart (the reference's fp32 autograd ends 9 % of the largest move away from its fp64 trajectory after
    these five steps), so each update is compared with the fp64 one from where the trainer stood."""
    from cirkit_amd.training_squared import HipSquaredTrainer

    lr = 1e-4
    plan_c, plan_z, tensors = _cfg5()
    tr = HipSquaredTrainer(plan_c, tensors, plan_z=plan_z, device=hip_device, optimizer="sgd", lr=lr)
    before = [dict(tensors)]

    def check(where, ll, B, gB, x):
        p = before[0]
        o64 = _sq_oracle(plan_c, plan_z, p, x)
        assert abs(float(ll[0]) - (o64[0] - B * o64[2])) <= 1e-4 * abs(o64[0] - B * o64[2]), (where, float(ll[0]), o64[0] - B * o64[2])
        g64, g32 = _sq_grad(o64, B, gB), _sq_grad(_sq_oracle(plan_c, plan_z, p, x, torch.float32), B, gB)
        got = tr.parameters()
        for k in p:
            ref = p[k].astype(np.float64) - lr * g64[k]
            ulp = 1.2e-7 * max(1.0, float(np.abs(ref).max()))
            err = float(np.abs(got[k] - ref).max())
            assert err <= lr * _sq_bound(g64[k], g32[k]) + 2 * ulp, (where, k, err, lr * float(np.abs(g64[k]).max()))
        before[0] = got

    _drive(tr, _STEPS, _sq_batch, check, monkeypatch, step=True)
    assert tr.step_count == len(_STEPS)
