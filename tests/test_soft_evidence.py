"""Soft (likelihood) evidence on the GPU (`HipCircuit.soft_evidence_log_prob`, `HipCircuit.soft_posterior_marginals`,
cirkit_amd/soft_evidence.py, cirkit_amd/csrc/ck_soft.hip; DESIGN.md section 11, "Soft evidence").

The reference has no such query.  The fp64 restatement of the contract (tests/soft_restatement.py) is pinned on the CPU
against brute force and central differences (tests/test_soft_restatement.py); here the GPU is compared with it.

GPU tolerance, the project's rule: ``max |got - want| / (1 + |want|)`` over the finite ``want`` of the fp64 restatement must be
within 4 x the same figure of the restatement run in fp32 on the test's own plan and evidence, at least 1e-6, computed and
printed by the test before it asserts; where ``want`` is -inf, so is ``got``.  Posteriors: the maximum absolute error under the
same 4 x yardstick, at least 1e-6; ``|sum_c p - 1|`` within 4 x the larger of that yardstick and the fp32 restatement's own
figure, as tests/test_posterior_marginals.py bounds it.  Every yardstick enters its bound capped at 1e-4, so that a loose one
cannot hide a failure (the restatement alone meets the cap on the hazard: tests/test_soft_restatement.py; its fp32 row sums at
config 2 do not -- 1.4e-4, the rounding of its own fp32 flow pass -- and count as 1e-4).  Measured yardsticks and GPU errors:
DESIGN.md section 11, "Soft evidence".
"""
import numpy as np
import pytest
import torch

from posterior_restatement import _log_table
from soft_restatement import soft_restated
from test_interval import _templated
from test_mpe import _case, _hc
from test_posterior_marginals import _states

CAP = 1e-4
ROWS = (1, 33, 70)
KINDS = ["dense", "channel", "onehot", "three", "dead"]
PLANS = ["kat_bernoulli_f0o0", "binomial_qg6x6_k4", "quadtree_4x4_kron_k3", "plan_quadgraph_1x4x4_cp", "quadgraph_6x6_tucker_k4",
         "plan_clt_mixed6_cp", "cat17_k3", "cat256_k32", "cat256_k64"]


def _plan(name, logit_std=None):
    """The golden cases by name; cat17_k3 (generic path, 17 states) and cat256_k32 (matrix-core path, K = 32) of
    tests/test_interval.py; cat256_k64: the latter's template with 64 units (matrix-core path, K = 64)."""
    if name == "cat256_k64":
        from cirkit_amd.initializers import init_plan_tensors
        from cirkit_amd.templates import image_data

        plan = image_data((1, 4, 4), region_graph="quad-tree-2", input_layer="categorical", num_input_units=64,
                          sum_product_layer="cp", num_sum_units=64)
        return plan, init_plan_tensors(plan, seed=5)
    if name in ("cat256_k32", "cat17_k3"):
        return _templated(name, logit_std)
    return _case(name)


def _soft(plan, every: int = 1) -> list[int]:
    """Every `every`-th variable a discrete layer reads."""
    return [int(v) for v in np.nonzero(_states(plan) > 0)[0]][::every]


def least_likely_states(plan, tensors, soft) -> np.ndarray:
    """(S,) per soft variable the state whose best unit is worst: argmin_c max_k table[k, c] of its first input fold."""
    from oracle.torch_oracle import as_torch, eval_param

    tt = {k: v.double() for k, v in as_torch(tensors).items()}
    out = np.zeros(len(soft), dtype=np.int64)
    todo = {v: i for i, v in enumerate(soft)}
    for l in plan.layers:
        if l.inputs is None and l.type in ("categorical", "binomial") and todo:
            tab = _log_table(l, {pn: eval_param(pg, tt) for pn, pg in l.params.items()}, np.float64)
            for f, v in enumerate(l.scope_idx[:, 0]):
                if int(v) in todo:
                    out[todo.pop(int(v))] = int(np.argmin(tab[f].max(axis=0)))
    return out


def evidence(plan, tensors, soft, B, kind, seed=0) -> np.ndarray:
    """(B, S, C) float64 log-likelihoods holding fp32 values.  dense: N(0, 1); channel: -(c - y)^2 / 8 around a random y;
    onehot: one state of weight 1; three: three live states of random weight; dead: dense, one variable without a live state
    in every third row; hazard_onehot / hazard_channel: onehot / channel centred on each variable's least likely state."""
    rng = np.random.default_rng(seed)
    states = _states(plan)[soft]
    S, C = len(soft), int(states.max())
    c = np.arange(C)[None, None, :]
    if kind in ("dense", "dead"):
        ll = rng.normal(size=(B, S, C))
        if kind == "dead":
            ll[::3, int(rng.integers(0, S)), :] = -np.inf
    elif kind in ("channel", "hazard_channel"):
        y = rng.integers(0, states, size=(B, S)) if kind == "channel" else np.broadcast_to(least_likely_states(plan, tensors, soft), (B, S))
        ll = -((c - y[:, :, None]) ** 2) / 8.0
    elif kind in ("onehot", "hazard_onehot"):
        y = rng.integers(0, states, size=(B, S)) if kind == "onehot" else np.broadcast_to(least_likely_states(plan, tensors, soft), (B, S))
        ll = np.where(c == y[:, :, None], 0.0, -np.inf)
    elif kind == "three":
        ll = np.full((B, S, C), -np.inf)
        for n in range(B):
            for s in range(S):
                live = rng.choice(int(states[s]), size=min(3, int(states[s])), replace=False)
                ll[n, s, live] = rng.normal(size=len(live))
    else:
        raise ValueError(kind)
    return ll.astype(np.float32).astype(np.float64)


def hard_evidence(plan, B, seed=0) -> np.ndarray:
    """(B, D) float64: a third of the entries missing (NaN), the rest a state of a discrete variable or a draw of a Gaussian."""
    rng = np.random.default_rng(seed + 1000)
    states = _states(plan)
    x = np.where(states > 0, rng.integers(0, np.maximum(states, 1), size=(B, plan.num_variables)),
                 rng.normal(size=(B, plan.num_variables)).astype(np.float32))
    x[rng.random(x.shape) < 1 / 3] = np.nan
    return x


def to_device(plan, x, dev):
    """The hard evidence as `forward` takes it: fp32 with NaN for a circuit with a Gaussian layer, else int64 with -1."""
    if (_states(plan) == 0).any():
        return torch.from_numpy(x).to(torch.float32).to(dev)
    return torch.from_numpy(np.where(np.isnan(x), -1, x)).to(torch.int64).to(dev)


def rel_error(got: np.ndarray, want: np.ndarray) -> float:
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        return float((np.abs(got.astype(np.float64) - want)[fin] / (1 + np.abs(want[fin]))).max())


class Reference:
    """The fp64 restatement of one (plan, evidence) and the bounds its fp32 twin gives; computed once, shared by the checks."""

    def __init__(self, plan, tensors, ll, x, soft):
        self.want = soft_restated(plan, tensors, ll, x, soft)
        y32 = soft_restated(plan, tensors, ll, x, soft, dtype=np.float32)
        self.live = np.isfinite(self.want["logev"])
        self.yard = rel_error(y32["y"], self.want["y"])
        p32, p64 = y32["p"][self.live].astype(np.float64), self.want["p"][self.live]
        self.yard_p = float(np.abs(p32 - p64).max()) if self.live.any() else 0.0
        self.yard_sum = float(np.abs(p32.sum(2) - 1).max()) if self.live.any() else 0.0
        print(f"  fp32-restatement yardsticks: log Z {self.yard:.3e}, posteriors {self.yard_p:.3e}, |sum_c p - 1| {self.yard_sum:.3e}")
        # (capped: a loose yardstick cannot hide a failure)
        self.bound = max(4 * min(self.yard, CAP), 1e-6)
        self.bound_p = max(4 * min(self.yard_p, CAP), 1e-6)
        self.bound_sum = max(self.bound_p, 4 * min(self.yard_sum, CAP), 1e-6)

    def check_log_prob(self, got: torch.Tensor, rows=slice(None)) -> float:
        want = self.want["y"][rows]
        got = got.cpu().numpy()
        assert got.shape == want.shape and got.dtype == np.float32, (got.shape, want.shape)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(got == -np.inf, want == -np.inf)
        assert not (got == np.inf).any()
        e = rel_error(got, want)
        print(f"  GPU log Z error {e:.3e} (bound {self.bound:.3e})")
        assert e <= self.bound, (e, self.bound)
        return e

    def check_posteriors(self, p: torch.Tensor, logev: torch.Tensor, rows=slice(None)) -> float:
        want, live = self.want["p"][rows], self.live[rows]
        p, logev = p.cpu().numpy(), logev.cpu().numpy()
        assert p.shape == want.shape and p.dtype == np.float32, (p.shape, want.shape)
        assert np.isnan(p[~live]).all() and np.isfinite(p[live]).all()
        wl = self.want["logev"][rows]
        assert np.array_equal(np.isnan(logev), np.isnan(wl)) and np.array_equal(logev == -np.inf, wl == -np.inf)
        assert rel_error(logev, wl) <= self.bound
        if not live.any():
            return 0.0
        e = float(np.abs(p[live].astype(np.float64) - want[live]).max())
        s = float(np.abs(p[live].astype(np.float64).sum(2) - 1).max())
        print(f"  GPU posterior error {e:.3e} (bound {self.bound_p:.3e}), |sum_c p - 1| {s:.3e} (bound {self.bound_sum:.3e})")
        assert e <= self.bound_p, (e, self.bound_p)
        assert s <= self.bound_sum, (s, self.bound_sum)
        assert (p[live] >= 0).all()
        return e


def _run_both(hc, ll_d, x_d, soft, **kw):
    lp = hc.soft_evidence_log_prob(ll_d, x_d, soft_vars=soft, **kw)
    p, lv = hc.soft_posterior_marginals(ll_d, x_d, soft_vars=soft, return_log_evidence=True, **kw)
    return lp, p, lv


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.gpu
def test_soft_surface(hip_device):
    from cirkit_amd import _capi as capi
    from cirkit_amd.circuit import HipCircuit
    from test_soft_restatement import NEW_ENTRY_POINTS

    lib = capi.load()
    for n in NEW_ENTRY_POINTS:
        assert hasattr(lib, n) and n in capi.SIGNATURES
    assert lib.ck_abi_version() == 51
    assert callable(HipCircuit.soft_evidence_log_prob) and callable(HipCircuit.soft_posterior_marginals)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", PLANS)
def test_gpu_soft_evidence_equals_restatement(hip_device, name, kind):
    plan, tensors = _plan(name)
    hc = _hc(plan, tensors, hip_device)
    templated = name.startswith("cat")
    B = ROWS[-1] if templated else ROWS[1]
    soft = _soft(plan)
    if not templated and plan.num_variables > 6:  # some variables stay hard evidence
        soft = soft[::2]
    ll = evidence(plan, tensors, soft, B, kind, seed=4)
    x = hard_evidence(plan, B, seed=4)
    ref = Reference(plan, tensors, ll, x, soft)
    ll_d, x_d = torch.from_numpy(ll).to(hip_device), to_device(plan, x, hip_device)
    lp, p, lv = _run_both(hc, ll_d, x_d, soft)
    ref.check_log_prob(lp)
    ref.check_posteriors(p, lv)
    dead = ~np.isfinite(ref.want["y"][:, 0, 0])
    if kind == "dead":  # only the rows with a variable without a live state are -inf
        assert dead[::3].all() and not dead[np.arange(B) % 3 != 0].any()
    else:
        assert not dead.any()
    if templated and kind == "dense":  # the other row counts (ragged row tiles): the same rows, on their own
        for n in ROWS[:-1]:
            lp, p, lv = _run_both(hc, ll_d[:n], x_d[:n], soft)
            ref.check_log_prob(lp, slice(0, n))
            ref.check_posteriors(p, lv, slice(0, n))
    hc.check_inputs()


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_soft_evidence_on_the_flagship_circuit(hip_device, kind):
    """cfg2_qt784 (784 variables of 256 states, 32 units) at 33 rows, soft on every 8th variable, the others observed or
    missing."""
    plan, tensors = _case("cfg2_qt784")
    hc = _hc(plan, tensors, hip_device)
    soft = _soft(plan, 8)
    ll = evidence(plan, tensors, soft, 33, kind, seed=5)
    x = hard_evidence(plan, 33, seed=5)
    ref = Reference(plan, tensors, ll, x, soft)
    lp, p, lv = _run_both(hc, torch.from_numpy(ll).to(hip_device), to_device(plan, x, hip_device), soft)
    ref.check_log_prob(lp)
    ref.check_posteriors(p, lv)


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["hazard_onehot", "hazard_channel"])
@pytest.mark.parametrize("name", ["binomial_qg6x6_k4", "cat256_k32"])
def test_gpu_soft_evidence_where_the_table_is_in_a_far_tail(hip_device, name, kind):
    """Evidence centred on each variable's least likely state, Binomial-255 log-pmf tables and 256-state softmax rows with
    logit standard deviation 30: the product of the two shifted exponentials underflows to 0 there (-inf from a plain
    log-einsum-exp); the exact recomputation below 2^-60 keeps the same bound, with no -inf where the restatement is finite."""
    plan, tensors = _plan(name, logit_std=30.0) if name == "cat256_k32" else _plan(name)
    hc = _hc(plan, tensors, hip_device)
    B = ROWS[1]
    soft = _soft(plan)
    ll = evidence(plan, tensors, soft, B, kind, seed=6)
    ref = Reference(plan, tensors, ll, None, soft)
    assert np.isfinite(ref.want["y"]).all()
    lp, p, lv = _run_both(hc, torch.from_numpy(ll).to(hip_device), None, soft)
    assert bool(torch.isfinite(lp).all())
    ref.check_log_prob(lp)
    ref.check_posteriors(p, lv)


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["plan_quadgraph_1x4x4_cp", "binomial_qg6x6_k4", "cat256_k32"])
def test_gpu_soft_evidence_identities(hip_device, name):
    """Point evidence, missing values, intervals and `posterior_marginals` are special cases: each GPU query against the
    other, within the bound of the restatement's yardstick on the same input (not bitwise: the sum changes the rounding)."""
    plan, tensors = _plan(name)
    D, B = plan.num_variables, ROWS[1]
    states = _states(plan)
    hc = _hc(plan, tensors, hip_device)
    z = _hc(plan, tensors, hip_device, fuse=False, pad_units=False, use_graph=False)
    soft = _soft(plan)[::2]
    S, C = len(soft), int(states[soft].max())
    rng = np.random.default_rng(7)
    x = rng.integers(0, states, size=(B, D))
    x[rng.random((B, D)) < 1 / 9] = -1
    x_d = torch.from_numpy(x).to(hip_device)
    c = np.arange(C)[None, None, :]
    xs = x.astype(np.float64)
    xs[xs < 0] = np.nan

    def close(got, want, ref):
        got, want = got.cpu().numpy(), want.cpu().numpy().astype(np.float64)
        assert np.array_equal(got == -np.inf, want == -np.inf)
        e = rel_error(got, want)
        print(f"  identity error {e:.3e} (bound {ref.bound:.3e})")
        assert e <= ref.bound, (e, ref.bound)

    # one-hot at x: the forward of x (a missing soft variable keeps weight 1 everywhere)
    xv = x[:, soft]
    ll = np.where((c == xv[:, :, None]) | (xv[:, :, None] < 0), 0.0, -np.inf)
    ref = Reference(plan, tensors, ll, xs, soft)
    got = hc.soft_evidence_log_prob(torch.from_numpy(ll).to(hip_device), x_d, soft_vars=soft)
    ref.check_log_prob(got)
    close(got, z(x_d).clone(), ref)
    # weight 1 everywhere: the forward with the soft variables integrated; the posteriors of `posterior_marginals`
    ll = np.zeros((B, S, C))
    ref = Reference(plan, tensors, ll, xs, soft)
    ll_d = torch.from_numpy(ll).to(hip_device)
    got = hc.soft_evidence_log_prob(ll_d, x_d, soft_vars=soft)
    ref.check_log_prob(got)
    close(got, z(x_d, integrate_vars=soft).clone(), ref)
    p, lv = hc.soft_posterior_marginals(ll_d, x_d, soft_vars=soft, return_log_evidence=True)
    ref.check_posteriors(p, lv)
    pm, pm_lv = hc.posterior_marginals(x_d, soft, return_log_evidence=True)
    assert tuple(p.shape) == tuple(pm.shape)
    e = float((p - pm).abs().max())
    print(f"  posteriors against posterior_marginals {e:.3e} (bound {ref.bound_p:.3e})")
    assert e <= ref.bound_p, (e, ref.bound_p)
    close(lv[:, None, None], pm_lv[:, None, None], ref)
    # 0 inside [lo, hi], -inf outside: interval_log_prob
    a, b = rng.integers(0, states[soft], size=(B, S)), rng.integers(0, states[soft], size=(B, S))
    a, b = np.minimum(a, b), np.maximum(a, b)
    ll = np.where((c >= a[:, :, None]) & (c <= b[:, :, None]), 0.0, -np.inf)
    lo, hi = x.copy(), x.copy()
    lo[:, soft], hi[:, soft] = a, b
    ref = Reference(plan, tensors, ll, xs, soft)
    got = hc.soft_evidence_log_prob(torch.from_numpy(ll).to(hip_device), x_d, soft_vars=soft)
    ref.check_log_prob(got)
    close(got, hc.interval_log_prob(torch.from_numpy(lo).to(hip_device), torch.from_numpy(hi).to(hip_device)), ref)
    hc.check_inputs()


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["plan_quadgraph_1x4x4_cp", "cat256_k32", "plan_clt_mixed6_cp"])
def test_gpu_soft_evidence_bad_rows_and_chunking(hip_device, name):
    """A NaN in one read entry, a +inf in another row and an out-of-range hard category in a third make exactly those rows
    NaN, for every chunking; all the other rows are bit-identical across the chunkings.  A NaN at c >= states(v) changes
    nothing."""
    plan, tensors = _plan(name)
    hc = _hc(plan, tensors, hip_device)
    B = ROWS[-1]
    states = _states(plan)
    soft = _soft(plan)[::2]
    hard = [v for v in range(plan.num_variables) if states[v] > 0 and v not in soft]
    ll = evidence(plan, tensors, soft, B, "dense", seed=8)
    x = hard_evidence(plan, B, seed=8)
    clean = _run_both(hc, torch.from_numpy(ll).to(hip_device), to_device(plan, x, hip_device), soft)
    hc.check_inputs()
    assert all(bool(torch.isfinite(t).all()) for t in clean)
    ll[5, 0, 1], ll[40, len(soft) - 1, 0] = np.nan, np.inf
    x[62, hard[0]] = states[hard[0]]
    pad = np.full((B, len(soft), 3), np.nan)  # columns past every variable's states: never read
    ll_d, x_d = torch.from_numpy(np.concatenate([ll, pad], axis=2)).to(hip_device), to_device(plan, x, hip_device)
    nan_rows = torch.zeros(B, dtype=torch.bool, device=hip_device)
    nan_rows[[5, 40, 62]] = True
    res = []
    for r in (None, 1, 7):
        lp, p, lv = _run_both(hc, ll_d, x_d, soft, rows_per_chunk=r)
        with pytest.raises(IndexError):
            hc.check_inputs()
        assert bool(torch.isnan(lp[nan_rows]).all()) and bool(torch.isnan(p[nan_rows][:, :, : ll.shape[2]]).all())
        assert bool(torch.isnan(lv[nan_rows]).all())
        assert bool(torch.isfinite(lp[~nan_rows]).all()) and bool(torch.isfinite(p[~nan_rows]).all())
        assert bool(torch.isfinite(lv[~nan_rows]).all())
        assert bool((p[~nan_rows][:, :, ll.shape[2]:] == 0).all())
        res.append((lp[~nan_rows], p[~nan_rows], lv[~nan_rows]))
    for other in res[1:]:
        assert all(torch.equal(a, b) for a, b in zip(res[0], other))
    ok = ~nan_rows
    assert torch.equal(res[0][0], clean[0][ok]) and torch.equal(res[0][2], clean[2][ok])
    assert torch.equal(res[0][1][:, :, : ll.shape[2]], clean[1][ok])
    with pytest.raises(ValueError):
        hc.soft_evidence_log_prob(ll_d, x_d, soft_vars=soft, rows_per_chunk=0)


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.gpu
def test_gpu_soft_evidence_follows_the_parameters(hip_device):
    plan, tensors = _plan("cat256_k32")
    hc = _hc(plan, tensors, hip_device)
    soft = _soft(plan)
    B = ROWS[1]
    ll = evidence(plan, tensors, soft, B, "channel", seed=9)
    ll_d = torch.from_numpy(ll).to(hip_device)
    before = _run_both(hc, ll_d, None, soft)
    Reference(plan, tensors, ll, None, soft).check_log_prob(before[0])
    cat = plan.layers[0]
    name = [n for n in cat.params["probs"].nodes if n.op == "tensor"][0].config["tensor"]
    v = np.array(hc.store.export(name), dtype=np.float32)
    v = (v + 2.0 * np.random.default_rng(10).normal(size=v.shape)).astype(np.float32)
    hc.store.set(name, v)
    tensors = dict(tensors)
    tensors[name] = v
    lp, p, lv = _run_both(hc, ll_d, None, soft)
    assert not torch.equal(lp, before[0])
    ref = Reference(plan, tensors, ll, None, soft)
    ref.check_log_prob(lp)
    ref.check_posteriors(p, lv)
