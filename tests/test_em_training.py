"""EM training (`HipEMTrainer`, cirkit_amd/em.py; the M-step launch `ck_em_update`, cirkit_amd/csrc/ck_em.hip; DESIGN.md
section 11, "EM training").

The reference has no EM.  The fp64 restatement of the M-step (tests/em_restatement.py, pinned on the CPU by
tests/test_em_restatement.py) is the yardstick: the kernel alone is driven through `HipEMTrainer.apply` with statistics the
fp64 restatement computed, the whole step through `step` against statistics + M-step restated.

What is compared is what the raw tensors MEAN (`normalised_parameters`: the oracle's fp64 evaluation of every parameter graph
on the downloaded raw tensors); for bare-tensor weights and Gaussian means that IS the raw value.  GPU tolerance: `_bound`'s
rule of tests/test_posterior_marginals.py -- the error of a parameter is max |got - want| / (1 + |want|), the yardstick that
error of the restatement run in float32 on the test's own input, the GPU must be within 4 x the yardstick, at least 1e-6.

Row lengths: ck_em.hip takes rows of up to 256 entries one wave per row (four rows per workgroup) and longer rows one
workgroup per row, re-reading the row from L2 (no single-pass limit); the cases below sit on both sides of 64 (one entry per
lane), of 256 and go up to 4096.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from em_restatement import _rows, em_restated, normalised_parameters
from statistics_restatement import statistics_restated
from test_em_restatement import TEMPLATES, _any, mean_ll
from test_expected_statistics import SMALL, _random_x, _small
from test_mpe import PLANS

# the fixtures of tests/test_mpe.py the trainer refuses, with the op behind the refusal
REFUSED = {"kat_gaussian_f1o1": "stddev' with ops ['tensor']", "binomial_qg6x6_k4": "matmul", "pd_gauss_6x6_k4": "matmul"}
# (cfg2_qt784 is accepted -- test_refusals_come_before_anything_is_allocated checks it -- but is the workload's own shape: its
# restatement alone takes 7 s per pattern, and the GPU tests keep to the small plans, as tests/test_expected_statistics.py does)
STEP_PLANS = list(SMALL) + list(TEMPLATES) + [p for p in PLANS if p not in REFUSED and p != "cfg2_qt784"]
NAN_BITS = 0x7FC0DEAD
GUARD = 64


def _plan(name):
    return _small(name) if name in SMALL else _any(name)


def _row_plan(L, bare=False):
    """categorical (L units) -> sum (3 units, rows of L entries) -> CP-T over two variables: sum weights of row length L."""
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.templates import InputSpec, build_plan, random_binary_tree

    act = {"sum_activation": "none", "input_activation": "none"} if bare else {}
    plan = build_plan(random_binary_tree(2), input_layer=InputSpec("categorical", 2), num_input_units=L, num_sum_units=3, **act)
    if not bare:
        return plan, init_plan_tensors(plan, seed=11)
    rng = np.random.default_rng(12)
    tensors = {}
    for l in plan.layers:
        for g in l.params.values():
            n = g.nodes[0].config["tensor"]
            t = rng.random(plan.tensors[n][0]) + 0.1
            t = (t / t.sum(axis=-1, keepdims=True)).astype(np.float32)
            tensors[n] = np.log(t) if l.inputs is None else t
    return plan, tensors


@functools.lru_cache(maxsize=None)
def _binomial_long():
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.templates import InputSpec, build_plan, random_binary_tree

    plan = build_plan(random_binary_tree(3), input_layer=InputSpec("binomial", 300), num_input_units=5, num_sum_units=3)
    return plan, init_plan_tensors(plan, seed=13)


def _evidence(plan, B, seed):
    gauss = any(l.type == "gaussian" for l in plan.layers)
    return _random_x(plan, B, np.random.default_rng(seed)) * (0.5 if gauss else 1)


def _pattern(kind, plan, x, rng):
    """(evidence with sentinels, missing variables) of a missing pattern: none, a random half of the variables, per-row."""
    D = plan.num_variables
    if kind == "half":
        return x, sorted(rng.choice(D, size=D // 2, replace=False).tolist())
    if kind == "sentinels":
        gauss = any(l.type == "gaussian" for l in plan.layers)
        m = rng.random(x.shape) < 1.0 / 3.0
        m[m.all(axis=1), 0] = False
        x = np.where(m, np.nan if gauss else -1.0, x)
    return x, []


def _to_device(plan, x, dev):
    gauss = any(l.type == "gaussian" for l in plan.layers)
    return torch.from_numpy(x.astype(np.float32) if gauss else x.astype(np.int64)).to(dev)


def _errors(plan, got: dict, want: dict) -> dict:
    g, w = normalised_parameters(plan, got), normalised_parameters(plan, want)
    out = {}
    for key in w:
        assert g[key].shape == w[key].shape and np.isfinite(g[key]).all(), key
        out[key] = float((np.abs(g[key] - w[key]) / (1 + np.abs(w[key]))).max())
    return out


def _assert_close(plan, got, want64, want32, what=""):
    yard, err = _errors(plan, want32, want64), _errors(plan, got, want64)
    print(f"  {what} yardstick {max(yard.values()):.3e}, GPU error {max(err.values()):.3e}")
    for key, e in err.items():
        assert e <= max(4 * yard[key], 1e-6), (key, e, yard[key])


@functools.lru_cache(maxsize=None)
def _step_reference(name, pattern, step_size=1.0, pseudocount=0.0, steps=1):
    """(evidence, missing, [per step: fp64 new tensors, fp32 new tensors, fp64 mean log evidence before the step])."""
    plan, tensors = _plan(name)
    x, missing = _pattern(pattern, plan, _evidence(plan, 70, 31), np.random.default_rng(32))
    t64, t32, out = dict(tensors), dict(tensors), []
    for _ in range(steps):
        r64 = statistics_restated(plan, t64, x, missing)
        r32 = statistics_restated(plan, t32, x, missing, dtype=np.float32)
        t64 = {**t64, **em_restated(plan, t64, r64, step_size, pseudocount)}
        t32 = {**t32, **em_restated(plan, t32, r32, step_size, pseudocount, dtype=np.float32)}
        out.append((t64, t32, float(r64["logev"][np.isfinite(r64["logev"])].mean())))
    return x, missing, out


def _trainer(plan, tensors, dev, **kw):
    from cirkit_amd.em import HipEMTrainer

    return HipEMTrainer(plan, tensors, device=dev, **kw)


# ------------------------------------------------------------------------------------------------------------ CPU
def _with_graph(plan, j, pn, mutate):
    """A deep copy of `plan` whose parameter `pn` of layer j went through `mutate(graph)`."""
    import copy

    plan = copy.deepcopy(plan)
    mutate(plan.layers[j].params[pn])
    return plan


def test_refusals_come_before_anything_is_allocated():
    """Every refusal is raised by the constructor on a machine without a device: nothing was allocated or launched."""
    from cirkit_amd.em import HipEMTrainer, em_jobs
    from cirkit_amd.plan import IDX_ARRAY, FoldIndex

    plan, tensors = _plan("cfg1_rbt8")
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="step_size"):
            HipEMTrainer(plan, tensors, step_size=bad)
    for bad in (-1e-3, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="pseudocount"):
            HipEMTrainer(plan, tensors, pseudocount=bad)
    for name, op in REFUSED.items():
        p, t = _plan(name)
        with pytest.raises(NotImplementedError, match=r"layer \d+ \(") as e:
            HipEMTrainer(p, t)
        assert op in str(e.value), (name, str(e.value))
    for op in ("clamp", "softplus"):  # an activation EM cannot invert
        p = _with_graph(plan, 1, "weight", lambda g: setattr(g.nodes[1], "op", op))
        with pytest.raises(NotImplementedError, match=rf"layer 1 \(sum\), parameter 'weight' with ops \['tensor', '{op}'\]"):
            HipEMTrainer(p, tensors)
    p = _with_graph(plan, 2, "weight", lambda g: setattr(g.nodes[0], "op", "pointer"))
    with pytest.raises(NotImplementedError, match=r"layer 2 \(cpt\).*pointer"):
        HipEMTrainer(p, tensors)
    F = plan.layers[1].num_folds

    def reverse(g):
        g.nodes[1].inputs[0] = FoldIndex(IDX_ARRAY, [0], np.arange(F)[::-1].copy())

    with pytest.raises(NotImplementedError, match=r"identity fold indices.*layer 1 \(sum\)"):
        HipEMTrainer(_with_graph(plan, 1, "weight", reverse), tensors)
    two = _plan("kat_bernoulli_f0o0")[0]
    two = _with_graph(two, 1, "probs", lambda g: g.nodes[0].config.__setitem__("tensor", "t0"))
    with pytest.raises(NotImplementedError, match=r"'t0' is read by layer 0 .* and by layer 1 "):
        HipEMTrainer(two, _plan("kat_bernoulli_f0o0")[1])
    sq = _with_graph(plan, 1, "weight", lambda g: None)
    sq.semiring = "complex-lse-sum"  # (a squared circuit: `sampling.check_plan`'s refusal)
    with pytest.raises(ValueError, match="lse-sum"):
        HipEMTrainer(sq, tensors)
    assert all(len(em_jobs(_plan(n)[0])) > 0 for n in STEP_PLANS + ["cfg2_qt784"])  # everything else is accepted


def test_em_entry_points_are_exported_at_abi_51():
    from cirkit_amd import _capi as capi

    lib = capi.load()
    assert lib.ck_abi_version() == 51
    for n in ("ck_em_update", "ck_em_job_blocks"):
        assert hasattr(lib, n) and n in capi.SIGNATURES
    assert ctypes.sizeof(capi.EMJob) == 72
    assert [lib.ck_em_job_blocks(capi.CK_EM_ROW_SOFTMAX, 10, n) for n in (1, 256, 257)] == [3, 3, 10]
    assert lib.ck_em_job_blocks(capi.CK_EM_GAUSSIAN, 257, 3) == 2


def _job(capi, **kw):
    j = capi.EMJob()
    base = dict(raw=64, raw2=None, stats=64, support=None, rows=4, len=8, kind=capi.CK_EM_ROW_SOFTMAX, k=0, raw_log=1, lo=0.0,
                hi=1.0, block_begin=0)
    for k, v in {**base, **kw}.items():
        setattr(j, k, v)
    return j


def test_em_invalid_arguments_return_status_and_message():
    from cirkit_amd import _capi as capi

    lib = capi.load()
    p = 64  # (never dereferenced: validation comes before any launch)
    ok = (capi.EMJob * 1)(_job(capi))
    cases = [
        (None, p, 1, 1.0, 0.0, None), (ok, None, 1, 1.0, 0.0, None), (ok, p, 0, 1.0, 0.0, None),
        (ok, p, 1, 0.0, 0.0, None), (ok, p, 1, 1.5, 0.0, None), (ok, p, 1, float("nan"), 0.0, None),
        (ok, p, 1, 1.0, -0.1, None), (ok, p, 1, 1.0, float("inf"), None),
    ]
    for bad in (dict(kind=7), dict(raw=None), dict(stats=None), dict(rows=0), dict(len=0), dict(raw_log=0),
                dict(kind=capi.CK_EM_MIXING, k=0), dict(kind=capi.CK_EM_MIXING, k=3), dict(kind=capi.CK_EM_GAUSSIAN, len=3),
                dict(kind=capi.CK_EM_GAUSSIAN, len=4, raw2=p), dict(kind=capi.CK_EM_GAUSSIAN, len=3, raw2=p, lo=1.0, hi=1.0),
                dict(kind=capi.CK_EM_BINOMIAL, len=1), dict(block_begin=1)):
        cases.append(((capi.EMJob * 1)(_job(capi, **bad)), p, 1, 1.0, 0.0, None))
    cases.append(((capi.EMJob * 2)(_job(capi), _job(capi, block_begin=2)), p, 2, 1.0, 0.0, None))  # (the first job has 1 block)
    for args in cases:
        assert lib.ck_em_update(*args) == -1, args
        assert "ck_em_update" in lib.ck_last_error().decode()
        with pytest.raises(ValueError, match="ck_em_update"):
            capi.call("ck_em_update", *args)
    assert lib.ck_em_job_blocks(9, 1, 1) == -1 and "ck_em_job_blocks" in lib.ck_last_error().decode()


@pytest.mark.parametrize("name", ["em_bare", "em_softmax", "gauss_qt2_k4"])
def test_the_restatement_is_monotone_on_the_plans_of_the_gpu_monotonicity_test(name):
    """What test_gpu_five_steps_never_lower_the_likelihood relies on: the fp64 restatement alone, same plans, same seed."""
    plan, _ = _plan(name)
    x, missing, steps = _step_reference(name, "sentinels", steps=5)
    miss = np.isnan(x) if any(l.type == "gaussian" for l in plan.layers) else x < 0
    lls = [mean_ll(plan, _plan(name)[1], x, miss)] + [mean_ll(plan, t64, x, miss) for t64, _, _ in steps]
    assert lls[-1] > lls[0] and all(b >= a - 1e-9 for a, b in zip(lls, lls[1:])), lls


# ------------------------------------------------------------------------------------------------------------ GPU
class _Guarded:
    """An fp32 tensor of `shape` between two blocks of GUARD words holding a NaN bit pattern no kernel produces."""

    def __init__(self, value: np.ndarray, dev):
        n = int(value.size)
        self.bits = torch.full((2 * GUARD + n,), NAN_BITS, dtype=torch.int32, device=dev)
        self.out = self.bits[GUARD : GUARD + n].view(torch.float32).view(value.shape)
        self.out.copy_(torch.from_numpy(np.ascontiguousarray(value, dtype=np.float32)))

    def read(self) -> np.ndarray:
        b = self.bits.cpu()
        assert bool((b[:GUARD] == NAN_BITS).all()), "words BEFORE the tensor were overwritten"
        assert bool((b[-GUARD:] == NAN_BITS).all()), "words AFTER the tensor were overwritten"
        return b[GUARD:-GUARD].view(torch.float32).numpy().reshape(self.out.shape).copy()


def _synthetic_jobs(capi, rng):
    """(job fields, raw value(s), statistics, support) of small jobs of every kind on both sides of the row boundaries."""
    out = []
    for kind, ln, rows, is_log in [(0, 1, 5, 1), (0, 3, 7, 1), (0, 63, 5, 1), (0, 64, 4, 1), (0, 65, 6, 1), (0, 256, 5, 1),
                                   (0, 257, 3, 1), (0, 1000, 2, 1), (0, 4096, 2, 1), (0, 5000, 1, 1), (1, 3, 9, 0), (1, 257, 2, 0),
                                   (1, 40, 3, 1)]:
        raw = rng.normal(size=(rows, ln)) if is_log else rng.random((rows, ln)) + 0.05
        if ln > 2:
            raw[:, 1] = -np.inf if is_log else 0.0  # an entry outside the support
        N = rng.random((rows, ln)) * (raw > (-np.inf if is_log else 0))
        N[rows // 2] = 0  # a row without flow
        sup = (raw > (-np.inf if is_log else 0)).astype(np.float32)
        sup[rows // 2] = 0  # (and outside every support: the pseudocount does not reach it)
        out.append((dict(kind=kind, rows=rows, len=ln, raw_log=is_log), [raw], N, sup if kind == 0 else None))
    for K, H, is_log in [(3, 2, 1), (32, 2, 1), (5, 300, 1), (4, 3, 0)]:  # mixing: (F, K, H) against (F, K, H K)
        F = 2
        raw = rng.normal(size=(F, K, H)) if is_log else rng.random((F, K, H)) + 0.05
        N = np.zeros((F, K, H * K))
        k = np.arange(K)
        for h in range(H):
            N[:, k, h * K + k] = rng.random((F, K))
        N[0, K - 1] = 0
        out.append((dict(kind=capi.CK_EM_MIXING, rows=F * K, len=H, k=K, raw_log=is_log), [raw], N, (N > 0).astype(np.float32)))
    for units in (7, 300):
        s0 = rng.random(units) * 5 + 0.5
        mu = rng.normal(size=units) * 0.3
        var = rng.random(units) * 0.2
        var[1] = 0.0
        S = np.stack([s0, s0 * mu, s0 * (var + mu * mu)], axis=-1)
        S[2] = 0
        out.append((dict(kind=capi.CK_EM_GAUSSIAN, rows=units, len=3, lo=1e-5, hi=1.0), [rng.normal(size=units), rng.normal(size=units)],
                    S, None))
    for units, T in [(9, 255), (3, 299), (6, 1)]:
        N = rng.random((units, T + 1))
        N[0], N[1], N[2] = 0, 0, 0
        N[1, 0], N[2, T] = 2.0, 3.0  # p_hat = 0 and 1
        out.append((dict(kind=capi.CK_EM_BINOMIAL, rows=units, len=T + 1), [rng.normal(size=units)], N, None))
    return out


def _launch(capi, dev, specs, step, pseudo):
    """One `ck_em_update` over `specs` on fresh guarded copies of their raw tensors; returns the tensors read back."""
    lib = capi.load()
    arr = (capi.EMJob * len(specs))()
    keep, blocks = [], 0
    for a, (fields, raws, N, sup) in zip(arr, specs):
        g = [_Guarded(r, dev) for r in raws]
        st = torch.from_numpy(N.astype(np.float32)).to(dev)
        sp = None if sup is None else torch.from_numpy(sup).to(dev)
        keep.append((g, st, sp))
        for k, v in {**dict(raw2=None, support=None, k=0, raw_log=0, lo=0.0, hi=1.0), **fields}.items():
            setattr(a, k, v)
        a.raw, a.stats = g[0].out.data_ptr(), st.data_ptr()
        if len(g) > 1:
            a.raw2 = g[1].out.data_ptr()
        if sp is not None:
            a.support = sp.data_ptr()
        a.block_begin = blocks
        blocks += lib.ck_em_job_blocks(a.kind, a.rows, a.len)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    capi.call("ck_em_update", arr, table.data_ptr(), len(specs), step, pseudo, None)
    torch.cuda.synchronize(dev)
    return [[t.read() for t in g] for g, _, _ in keep]


@pytest.mark.gpu
def test_gpu_job_lists_are_guarded_bit_identical_and_close(hip_device):
    """Jobs of every kind and row length as ONE table and as tables of one job each: the same bits, nothing outside the
    tensors written, rows without flow and entries outside the support kept, and the row kinds within the bound of the
    restatement's own row formula (step_size 0.5, pseudocount 0.1)."""
    from cirkit_amd import _capi as capi

    specs = _synthetic_jobs(capi, np.random.default_rng(51))
    step, pseudo = 0.5, 0.1
    many = _launch(capi, hip_device, specs, step, pseudo)
    again = _launch(capi, hip_device, specs, step, pseudo)
    for i, (spec, got) in enumerate(zip(specs, many)):
        single = _launch(capi, hip_device, [spec], step, pseudo)[0]
        fields, raws, N, sup = spec
        for a, b, c, r in zip(got, single, again[i], raws):
            assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c, equal_nan=True), fields
            assert not np.isnan(a).any(), fields
        kind, r32 = fields["kind"], raws[0].astype(np.float32)
        if kind <= capi.CK_EM_MIXING:
            is_log = bool(fields["raw_log"])
            if kind == capi.CK_EM_MIXING:
                K, H = fields["k"], fields["len"]
                k = np.arange(K)
                N = np.stack([N[:, k, h * K + k] for h in range(H)], axis=-1)
                sup = N > 0
            elif sup is not None:
                sup = sup > 0
            want = _rows(r32.astype(np.float64), N.astype(np.float32), sup, is_log, step, pseudo, np.float64)
            w32 = _rows(r32, N.astype(np.float32), sup, is_log, step, pseudo, np.float32)
            th = (lambda t: np.exp(t)) if is_log else (lambda t: t)
            err = lambda t: float((np.abs(th(t.astype(np.float64)) - th(want)) / (1 + th(want))).max())  # noqa: E731
            assert err(got[0]) <= max(4 * err(w32), 1e-6), (fields, err(got[0]), err(w32))
            own = sup if sup is not None else r32 > (-np.inf if is_log else 0)  # (no mask: the support is the row's own)
            dead = ~(N.astype(np.float32).sum(-1) + pseudo * own.sum(-1) > 0)
            assert dead.any() or sup is None, fields
            assert np.array_equal(got[0][dead], r32[dead]), fields  # no mass: bit for bit
            if fields["len"] > 2 and kind != capi.CK_EM_MIXING:
                assert np.all(got[0][~dead][:, 1] == (-np.inf if is_log else 0.0)), fields
        elif kind == capi.CK_EM_GAUSSIAN:
            assert got[0][2] == r32[2] and got[1][2] == raws[1].astype(np.float32)[2]  # no flow: kept
            assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()  # (var_hat = 0 at unit 1)
        else:
            assert got[0][0] == r32[0] and np.isfinite(got[0]).all()


APPLY_CASES = [("rows", L, False) for L in (1, 3, 63, 64, 65, 256, 257, 1000, 4096)] + [("rows", 3, True), ("rows", 64, True), ("rows", 257, True)] + \
    [(n, 0, False) for n in ("gauss_qt2_k4", "binom_qt2_k4", "binom_long", "qg_cp_k3", "qt2_tucker_k32", "kat_bernoulli_f0o1")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,L,bare", APPLY_CASES)
def test_gpu_kernel_alone_through_apply(hip_device, name, L, bare):
    """`apply` on the fp64 restatement's statistics, cast to fp32: the only device work under test is ck_em.hip."""
    from cirkit_amd.expected import ExpectedStatistics

    plan, tensors = _row_plan(L, bare) if name == "rows" else _binomial_long() if name == "binom_long" else _plan(name)
    x = _evidence(plan, 64, 52)
    res = statistics_restated(plan, tensors, x, [0])
    cast = {k: {j: v.astype(np.float32) for j, v in res[k].items()} for k in ("edge", "leaf")}
    want64 = {**tensors, **em_restated(plan, tensors, {**cast, "w": res["w"]})}
    want32 = {**tensors, **em_restated(plan, tensors, {**cast, "w": res["w"]}, dtype=np.float32)}
    tr = _trainer(plan, tensors, hip_device, pad_units=name != "rows")
    up = lambda d: {j: torch.from_numpy(v).to(hip_device) for j, v in d.items()}  # noqa: E731
    tr.apply(ExpectedStatistics(up(cast["edge"]), up(cast["leaf"]), [], None, None))
    got = tr.parameters()
    assert all(got[n].shape == tuple(plan.tensors[n][0]) for n in got)
    _assert_close(plan, got, want64, want32, f"{name} {L}")


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["none", "half", "sentinels"])
@pytest.mark.parametrize("name", STEP_PLANS)
def test_gpu_step_equals_restatement(hip_device, name, pattern):
    plan, tensors = _plan(name)
    x, missing, [(want64, want32, ll)] = _step_reference(name, pattern)
    tr = _trainer(plan, tensors, hip_device)
    got_ll = tr.step(_to_device(plan, x, hip_device), missing or None)
    assert got_ll.dim() == 0 and got_ll.device.type == "cuda"
    assert abs(float(got_ll) - ll) <= 1e-4 * (1 + abs(ll))
    _assert_close(plan, tr.parameters(), want64, want32, f"{name} {pattern}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["qt2_cp_k32", "qg_cp_k3", "gauss_qt2_k4"])
def test_gpu_step_leaves_no_stale_cache(hip_device, name):
    from oracle.torch_oracle import as_torch, evaluate_plan

    plan, tensors = _plan(name)
    x, _, _ = _step_reference(name, "none")
    xd = _to_device(plan, x, hip_device)
    tr = _trainer(plan, tensors, hip_device)
    hc = tr.circuit
    before = hc(xd).clone()
    st0 = hc.expected_statistics(xd)
    tr.step(xd)
    new = tr.parameters()
    y = hc(xd).cpu()
    want = evaluate_plan(plan, as_torch(new), xd.cpu())
    assert not torch.equal(y, before.cpu())
    assert float(((y - want).abs() / want.abs()).max()) <= 1e-4  # (the forward's own tolerance: __graft_entry__.smoke)
    st1 = hc.expected_statistics(xd)
    from test_mpe import _hc

    fresh = _hc(plan, new, hip_device).expected_statistics(xd)
    assert not torch.equal(st0.log_evidence, st1.log_evidence)
    assert float((st1.log_evidence - fresh.log_evidence).abs().max()) <= 1e-4 * (1 + float(fresh.log_evidence.abs().max()))
    assert float(st1.log_evidence.mean()) > float(st0.log_evidence.mean())


@pytest.mark.gpu
def test_gpu_rows_without_flow_stay_bit_identical(hip_device):
    plan, tensors = _plan("cfg1_rbt8")
    tr = _trainer(plan, tensors, hip_device)
    store = tr.circuit.store
    x = _to_device(plan, _evidence(plan, 64, 53), hip_device)
    bad = x.clone()
    bad[:, 2] = 99  # every row holds an observed category out of range: no live row
    raw0 = {n: store[n].clone() for n in store.names()}
    tr.step(bad)
    assert all(torch.equal(store[n], raw0[n]) for n in raw0)
    with pytest.raises(IndexError):
        tr.check_inputs()
    tr.check_inputs()
    # a point mass: unit 1 of every fold of the first sum layer is never chosen by the layer above, so it carries no flow
    plan, tensors = _plan("qg_cp_k3")
    j = next(j for j, l in enumerate(plan.layers) if l.type == "cpt")
    n = plan.layers[j].params["weight"].nodes[0].config["tensor"]
    t = dict(tensors)
    t[n] = np.array(t[n], dtype=np.float32)
    t[n][:, :, 1] = -np.inf
    tr = _trainer(plan, t, hip_device)
    assert tr.circuit._pad_info is not None  # (3 units padded to 32)
    x = _to_device(plan, _evidence(plan, 64, 54), hip_device)
    below = next(i for i, l in enumerate(plan.layers) if l.type == "sum")
    nb = plan.layers[below].params["weight"].nodes[0].config["tensor"]
    feeds = np.unique(np.asarray(tr.circuit._children[j])[..., 1])  # folds of the sum layer that the CP-T layer reads
    padded0 = {m: tr.circuit.store[m].clone() for m in tr.circuit.store.names()}
    tr.step(x)
    got = tr.parameters()
    assert all(got[m].shape == tuple(plan.tensors[m][0]) for m in got)
    assert np.array_equal(got[nb][feeds, 1], np.asarray(tensors[nb])[feeds, 1])  # no flow: the row is kept
    assert not np.array_equal(got[nb][feeds, 0], np.asarray(tensors[nb])[feeds, 0])
    assert np.all(got[n][:, :, 1] == -np.inf)
    for m, old in padded0.items():  # padded entries: still -inf / 0 exactly where they were
        new = tr.circuit.store[m]
        pad = torch.isinf(old) & (old < 0)
        assert bool((new[pad] == old[pad]).all()), m


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["qt2_cp_k32", "qg_cp_k3", "gauss_qt2_k4"])
def test_gpu_training_is_deterministic(hip_device, name):
    plan, tensors = _plan(name)
    x, _, _ = _step_reference(name, "sentinels")
    xd = _to_device(plan, x, hip_device)
    a, b = _trainer(plan, tensors, hip_device), _trainer(plan, tensors, hip_device)
    for _ in range(3):
        la, lb = a.step(xd), b.step(xd)
        assert torch.equal(la, lb)
    for n in a.circuit.store.names():
        assert torch.equal(a.circuit.store[n], b.circuit.store[n]), n


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["qt2_cpt_k64", "binom_qt2_k4"])
def test_gpu_accumulate_over_two_halves_is_one_step(hip_device, name):
    plan, tensors = _plan(name)
    x, missing, [(want64, want32, ll)] = _step_reference(name, "half")
    xd = _to_device(plan, x, hip_device)
    tr = _trainer(plan, tensors, hip_device)
    l0, l1 = tr.accumulate(xd[:33], missing), tr.accumulate(xd[33:], missing)
    assert abs((33 * float(l0) + 37 * float(l1)) / 70 - ll) <= 1e-4 * (1 + abs(ll))
    with pytest.raises(RuntimeError):
        tr.apply(tr.circuit.expected_statistics(xd, missing))
    tr.update()
    _assert_close(plan, tr.parameters(), want64, want32, name)
    raw = {n: tr.circuit.store[n].clone() for n in tr.circuit.store.names()}
    tr.update()  # (the sums were zeroed: nothing moves)
    assert all(torch.equal(tr.circuit.store[n], raw[n]) for n in raw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["qg_cp_k32", "gauss_qt2_k4", "binom_qt2_k4", "kat_bernoulli_f1o1"])
def test_gpu_step_size_and_pseudocount(hip_device, name):
    plan, tensors = _plan(name)
    x, missing, [(want64, want32, _)] = _step_reference(name, "sentinels", 0.5, 0.1)
    tr = _trainer(plan, tensors, hip_device, step_size=0.5, pseudocount=0.1)
    tr.step(_to_device(plan, x, hip_device))
    _assert_close(plan, tr.parameters(), want64, want32, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["em_bare", "em_softmax", "gauss_qt2_k4"])
def test_gpu_five_steps_never_lower_the_likelihood(hip_device, name):
    plan, tensors = _plan(name)
    x, _, steps = _step_reference(name, "sentinels", steps=5)
    miss = np.isnan(x) if any(l.type == "gaussian" for l in plan.layers) else x < 0
    xd = _to_device(plan, x, hip_device)
    tr = _trainer(plan, tensors, hip_device)
    lls = [mean_ll(plan, tensors, x, miss)]
    for t64, t32, _ in steps:
        tr.step(xd)
        lls.append(mean_ll(plan, tr.parameters(), x, miss))
        # the allowed drop: 4 x |fp32-restated - fp64-restated mean LL| of the step, at least 1e-6 (1 + |LL|)
        slack = max(4 * abs(mean_ll(plan, t32, x, miss) - mean_ll(plan, t64, x, miss)), 1e-6 * (1 + abs(lls[-1])))
        assert lls[-1] >= lls[-2] - slack, (lls, slack)
    assert lls[-1] > lls[0]
