"""Marginal MAP (`HipCircuit.marginal_map`, cirkit_amd/marginal_map.py, cirkit_amd/csrc/ck_mmap.hip).

The reference has no max semiring and no MAP query; these tests pin the GPU completion against a numpy fp64 restatement of
the contract (tests/mmap_restatement.py), and the restatement against brute force on the oracle where the circuit is small
enough to enumerate.  The bounds on the values are those `mpe`'s tests use: 1e-5 |ref| + 1e-5, and 1e-4 |ref| + 1e-3 on the
Binomial plans, whose device log-pmf table is fp32.

GPU evidence: `hc.sample(N, seed=SEED)`, then the sentinel in 30 % of the non-query entries (numpy rng MISS_SEED) and garbage
in the query columns.  With these two seeds the restatement alone flags at most 10 % of the rows of every case as near ties.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from conftest import load_case
from mmap_restatement import mmap_restated
from mpe_restatement import mpe_restated
from test_mpe import KAT, PLANS, _case, _discrete, _hc

SEED, MISS_SEED = 77, 5
TEMPLATED = {"qt2_cp_k32": ("cp", 32), "qt2_cpt_k64": ("cp-t", 64)}  # 4 x 4 Categorical-256: the 32- and 64-unit tiles
GPU_PLANS = PLANS + list(TEMPLATED)
QUERIES = ["lower_half", "every_other", "one", "all"]


@functools.lru_cache(maxsize=None)
def _plan(name):
    if name in TEMPLATED:
        from cirkit_amd.initializers import init_plan_tensors
        from cirkit_amd.templates import image_data

        sp, k = TEMPLATED[name]
        plan = image_data((1, 4, 4), "quad-tree-2", num_input_units=k, sum_product_layer=sp, num_sum_units=k)
        return plan, init_plan_tensors(plan, seed=5)
    return _case(name)


def _deterministic_case(D=6, C=4):
    """categorical -> sum (1 -> 1) -> CP-T (1 unit) over D variables: no unit mixes, so max and sum commute with it."""
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.templates import InputSpec, build_plan, fully_factorized

    plan = build_plan(fully_factorized(D), input_layer=InputSpec("categorical", C), num_input_units=1, num_sum_units=1)
    return plan, init_plan_tensors(plan, seed=3)


def _query(kind, D):
    q = np.zeros(D, dtype=bool)
    if kind == "lower_half":
        q[D // 2:] = True
    elif kind == "every_other":
        q[::2] = True
    elif kind == "one":
        q[D // 3] = True
    elif kind == "all":
        q[:] = True
    return q


def _oracle_marginal(plan, tensors, rows, hide):
    """fp64 log c of `rows` (n, D) with the entries `hide` marks integrated out."""
    from oracle.torch_oracle import as_torch, evaluate_plan

    tt = {k: v.double() for k, v in as_torch(tensors).items()}
    xs = torch.from_numpy(np.where(hide, 0, rows).astype(np.int64))
    return evaluate_plan(plan, tt, xs, integrate_mask=torch.from_numpy(np.ascontiguousarray(hide)))[:, 0, 0].numpy()


def _brute_force(plan, tensors, x, q, C):
    """(optimum (B,), argmax completion (B, D)) of log c(q, x_E) over the assignments of the query variables, by the oracle."""
    B, D = x.shape
    ids = np.nonzero(q)[0]
    worlds = np.array(list(itertools.product(range(C), repeat=len(ids))), dtype=np.int64).reshape(C ** len(ids), len(ids))
    hide = (x < 0) & ~q
    best, arg = np.full(B, -np.inf), np.where(hide, -1, x).astype(np.int64)
    for w in worlds:
        rows = x.copy()
        rows[:, ids] = w
        y = _oracle_marginal(plan, tensors, rows, hide)
        better = y > best  # (strict: the first of equal optima, in the order of the enumeration)
        best[better] = y[better]
        arg[np.ix_(better, ids)] = w
    return best, arg


# ------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("query", [(0, 2), (1, 3, 4), (0, 1, 2, 3, 4), ()])
@pytest.mark.parametrize("name", KAT)
def test_restatement_obeys_the_bound_chain_against_brute_force(name, query):
    plan, tensors = _case(name)
    D, B = 5, 24
    rng = np.random.default_rng(21)
    x = rng.integers(0, 2, size=(B, D)).astype(np.int64)
    x[B // 2:][rng.random((B - B // 2, D)) < 0.4] = -1  # the first half has no missing evidence, the second half has
    q = np.zeros(D, dtype=bool)
    q[list(query)] = True
    x[:, q] = 1 - x[:, q].clip(0)  # (garbage in the query columns: ignored)
    out, _, lv, lp, _ = mmap_restated(plan, tensors, x, q)
    assert np.isfinite(lv).all() and np.isfinite(lp).all()
    assert ((x[:, ~q] < 0) == (out[:, ~q] < 0)).all() and (out[:, ~q] == np.where(x[:, ~q] < 0, -1, x[:, ~q])).all()
    assert (out[:, q] >= 0).all()
    optimum, _ = _brute_force(plan, tensors, x, q, 2)
    assert (lv <= lp + 1e-12).all(), (lv - lp).max()
    assert (lp <= optimum + 1e-12).all(), (lp - optimum).max()
    own = _oracle_marginal(plan, tensors, out, out < 0)
    assert np.abs(lp - own).max() <= 1e-12


@pytest.mark.parametrize("name", KAT + ["cfg1_rbt8", "pd_gauss_6x6_k4", "binomial_qg6x6_k4", "quadgraph_6x6_tucker_k4"])
def test_restatement_with_every_variable_in_the_query_is_mpe(name):
    plan, tensors = _case(name)
    D, B = plan.num_variables, 16
    rng = np.random.default_rng(2)
    x = rng.normal(size=(B, D)) if not _discrete(plan).all() else rng.integers(0, 2, size=(B, D)).astype(np.float64)
    out, ch, lv, _, near = mmap_restated(plan, tensors, x, np.ones(D, dtype=bool))
    mo, mch, mlv, mnear = mpe_restated(plan, tensors, x, np.ones(D, dtype=bool))
    assert np.array_equal(out, mo) and np.array_equal(lv, mlv) and not (near & ~mnear).any()
    assert len(ch) == len(mch) and all(np.array_equal(a, b) for a, b in zip(ch, mch))


@pytest.mark.parametrize("name", KAT)
def test_restatement_with_an_empty_query_is_the_marginal(name):
    plan, tensors = _case(name)
    D, B = 5, 16
    rng = np.random.default_rng(3)
    x = rng.integers(0, 2, size=(B, D)).astype(np.int64)
    x[rng.random((B, D)) < 0.3] = -1
    out, ch, lv, lp, near = mmap_restated(plan, tensors, x, np.zeros(D, dtype=bool))
    assert np.array_equal(out, x.astype(np.float64)) and all((c == -1).all() for c in ch) and not near.any()
    want = _oracle_marginal(plan, tensors, x, x < 0)
    assert np.array_equal(lv, lp) and np.abs(lv - want).max() <= 1e-12


def test_restatement_is_the_exact_marginal_map_on_a_deterministic_circuit():
    from cirkit_amd.sampling import check_plan

    plan, tensors = _deterministic_case(6, 4)
    check_plan(plan)
    assert [l.type for l in plan.layers] == ["categorical", "sum", "cpt"]
    q = np.zeros(6, dtype=bool)
    q[[1, 2, 4]] = True
    x = np.full((4, 6), -1, dtype=np.int64)  # evidence on variable 0, variables 3 and 5 summed out
    x[:, 0] = np.arange(4)
    out, _, lv, lp, _ = mmap_restated(plan, tensors, x, q)
    optimum, arg = _brute_force(plan, tensors, x, q, 4)
    assert np.array_equal(out, arg.astype(np.float64))
    assert np.abs(lp - optimum).max() <= 1e-10 and np.abs(lv - optimum).max() <= 1e-10


def test_marginal_map_entry_points_are_exported_at_abi_51():
    from cirkit_amd import _capi as capi

    lib = capi.load()
    assert lib.ck_abi_version() == 51
    for n in ("ck_mmap_input_sum", "ck_mmap_up_input", "ck_mmap_up_sum", "ck_mmap_walk"):
        assert hasattr(lib, n) and n in capi.SIGNATURES


# ------------------------------------------------------------------------------------------------------------ GPU
def _bounds(plan):
    """(rtol, atol of the values, tie tolerance of a max fold): the Binomial log-pmf table the device evaluates is fp32 and
    off by up to ~1e-4 per entry, which a row sums over its variables (tests/test_mpe.py)."""
    return (1e-4, 1e-3, 1e-3) if any(l.type == "binomial" for l in plan.layers) else (1e-5, 1e-5, 1e-4)


def _leaf_tol(plan):
    """Tie tolerance of two categories of one input unit: twice the error of one table entry on the device.  Binomial: the
    ~1e-4 above.  Categorical: the log of an fp32 softmax against the oracle's fp64 one, a few ulp of the probability
    (~5e-7) -- not the error of a value that sums a sub-circuit, which is what the max folds' tolerance covers.  With the
    folds' tolerance here every row of the Binomial plan would count as a near tie: 36 variables of 256 states have some
    pair of neighbouring states within 1e-3 on every tree."""
    return 2e-4 if any(l.type == "binomial" for l in plan.layers) else 1e-6


def _close(plan, got, ref):
    rtol, atol, _ = _bounds(plan)
    return np.abs(got - ref) <= rtol * np.abs(ref) + atol


def _evidence(hc, plan, N, q, seed=SEED, miss_seed=MISS_SEED):
    """(x, masked): sampled evidence with the sentinel in 30 % of the non-query entries and garbage in the query columns,
    and the same batch with the sentinel in the query columns too (what the call is to see)."""
    x = hc.sample(N, seed=seed)
    D = plan.num_variables
    gauss = x.dtype == torch.float32
    miss = torch.from_numpy((np.random.default_rng(miss_seed).random((N, D)) < 0.3) & ~q).to(x.device)
    sentinel = float("nan") if gauss else -1
    x = torch.where(miss, torch.full((), sentinel, dtype=x.dtype, device=x.device), x)
    masked = x.clone()
    qd = torch.from_numpy(q).to(x.device)
    masked[:, qd] = sentinel
    x[:, qd] = 123.0 if gauss else 7
    return x, masked


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _check_against_restatement(plan, tensors, x, q, out, ch, lv, lp):
    rtol, atol, tol = _bounds(plan)
    x_np = x.cpu().numpy().astype(np.float64)
    out, ch = out.cpu().numpy(), [c.cpu().numpy() for c in ch]
    lv, lp = lv.cpu().numpy().astype(np.float64), lp.cpu().numpy().astype(np.float64)
    ro, rch, rlv, rlp, near = mmap_restated(plan, tensors, x_np, q, tol=tol, leaf_tol=_leaf_tol(plan))
    fin = np.isfinite(rlv)
    assert (np.isfinite(lv) == fin).all() and (np.isfinite(lp) == fin).all()
    ev, ep = np.abs(lv[fin] - rlv[fin]), np.abs(lp[fin] - rlp[fin])
    print(f"  log_value err {ev.max(initial=0):.3e}  log_prob err {ep.max(initial=0):.3e}"
          f"  |ref| {np.abs(rlv[fin]).max(initial=0):.4g}  near {near.mean():.3f}")
    assert _close(plan, lv[fin], rlv[fin]).all(), ev.max()
    assert _close(plan, lp[fin], rlp[fin]).all(), ep.max()
    disc = _discrete(plan)
    diff = ((out[:, disc] != ro[:, disc]) & ~(np.isnan(out[:, disc]) & np.isnan(ro[:, disc]))).any(axis=1)
    if (~disc).any():
        a, b = out[:, ~disc], ro[:, ~disc]
        diff |= ~((np.abs(a - b) <= 1e-5 * (1 + np.abs(b))) | (np.isnan(a) & np.isnan(b))).all(axis=1)
    for a, b in zip(ch, rch):
        diff |= (a != b).any(axis=0)
    assert not (diff & ~near).any(), np.nonzero(diff & ~near)[0][:8]
    assert diff.mean() <= 0.02, diff.mean()
    assert near.mean() <= 0.10, near.mean()
    return rlv, rlp


@functools.lru_cache(maxsize=None)
def _circuit(name, dev):
    return _hc(*_plan(name), dev)


@functools.lru_cache(maxsize=None)
def _run(name, kind, dev):
    """One call per (plan, query set), shared by the tests below: (hc, x, masked, q, out, choices, log_value, log_prob)."""
    plan, tensors = _plan(name)
    D = plan.num_variables
    N = 64 if name == "cfg2_qt784" else 200  # (200: no tile height, 64 / 128 / 256, divides it)
    q = _query(kind, D)
    hc = _circuit(name, dev)
    x, masked = _evidence(hc, plan, N, q)
    out, ch, lv, lp = hc.marginal_map(x, torch.from_numpy(q), return_choices=True, return_log_value=True,
                                      return_log_prob=True)
    torch.cuda.synchronize()
    return hc, x, masked, q, out, ch, lv, lp


@pytest.mark.gpu
@pytest.mark.parametrize("kind", QUERIES)
@pytest.mark.parametrize("name", GPU_PLANS)
def test_gpu_marginal_map_equals_restatement(hip_device, name, kind):
    plan, tensors = _plan(name)
    hc, x, masked, q, out, ch, lv, lp = _run(name, kind, hip_device)
    N, D = x.shape
    gauss = not _discrete(plan).all()
    assert out.shape == (N, D) and out.dtype == (torch.float32 if gauss else torch.int64) and out.device.type == "cuda"
    sums = [j for j, l in enumerate(plan.layers) if l.type in ("sum", "cpt", "tucker")]
    assert len(ch) == len(sums)
    for c, j in zip(ch, sums):
        assert c.dtype == torch.int32 and tuple(c.shape) == (plan.layers[j].num_folds, N)
    assert lv.shape == (N,) and lv.dtype == torch.float32 and lp.shape == (N,) and lp.dtype == torch.float32
    keep = torch.from_numpy(~q).to(hip_device)
    assert torch.equal(_bits(out[:, keep]), _bits(masked[:, keep]))  # evidence and summed-out entries: bit for bit
    _check_against_restatement(plan, tensors, x, q, out, ch, lv, lp)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg1_rbt8", "quadgraph_6x6_tucker_k4", "pd_gauss_6x6_k4", "cfg2_qt784"])
def test_gpu_marginal_map_over_every_variable_is_mpe_bit_for_bit(hip_device, name):
    plan, tensors = _plan(name)
    D = plan.num_variables
    N = 64 if name == "cfg2_qt784" else 200
    hc = _hc(plan, tensors, hip_device)
    x = hc.sample(N, seed=SEED)
    a = hc.marginal_map(x, range(D), return_choices=True, return_log_value=True)
    b = hc.mpe(x, range(D), return_choices=True, return_log_value=True)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[2]), _bits(b[2]))
    assert len(a[1]) == len(b[1]) and all(torch.equal(c, d) for c, d in zip(a[1], b[1]))
    assert bool(torch.isfinite(a[2]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg1_rbt8", "binomial_qg6x6_k4", "pd_gauss_6x6_k4", "qt2_cpt_k64"])
def test_gpu_marginal_map_with_an_empty_query_is_the_marginal(hip_device, name):
    plan, tensors = _plan(name)
    hc, x, masked, q, out, ch, lv, lp = _run(name, "none", hip_device)
    assert not q.any() and torch.equal(_bits(out), _bits(masked))
    assert all(bool((c == -1).all()) for c in ch)
    _, logev = hc.sample_conditional(masked, [], seed=1, return_log_evidence=True)
    for got in (lv, lp):
        assert _close(plan, got.cpu().numpy().astype(np.float64), logev.cpu().numpy().astype(np.float64)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", QUERIES)
@pytest.mark.parametrize("name", GPU_PLANS)
def test_gpu_marginal_map_bound_chain_and_self_consistency(hip_device, name, kind):
    plan, _ = _plan(name)
    hc, x, masked, q, out, ch, lv, lp = _run(name, kind, hip_device)
    rtol, atol, _ = _bounds(plan)
    assert bool((lv <= lp + rtol * lp.abs() + atol).all()), float((lv - lp).max())
    out2, lv2 = hc.marginal_map(out, [], return_log_value=True)  # the completion, with nothing left to maximise
    assert torch.equal(_bits(out2), _bits(out))
    assert _close(plan, lv2.cpu().numpy().astype(np.float64), lp.cpu().numpy().astype(np.float64)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lower_half", "every_other", "one"])
@pytest.mark.parametrize("name", KAT)
def test_gpu_log_prob_is_a_lower_bound_of_the_brute_force_optimum(hip_device, name, kind):
    plan, _ = _plan(name)
    hc, x, masked, q, out, ch, lv, lp = _run(name, kind, hip_device)
    ids = np.nonzero(q)[0]
    best = torch.full_like(lp, float("-inf"))
    hide = masked < 0
    hide[:, torch.from_numpy(q).to(hip_device)] = False
    for w in itertools.product(range(2), repeat=len(ids)):  # the enumerated completions, evaluated by the circuit itself
        rows = masked.clone()
        rows[:, ids] = torch.tensor(w, dtype=rows.dtype, device=hip_device)
        best = torch.maximum(best, hc(rows.clamp(min=0), integrate_vars=hide)[:, 0, 0])
    assert bool((lp <= best + 1e-5 * best.abs() + 1e-5).all()), float((lp - best).max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2_qt784", "pd_gauss_6x6_k4"])
def test_gpu_marginal_map_chunking_does_not_change_results(hip_device, name):
    plan, tensors = _plan(name)
    D, B = plan.num_variables, 100
    hc = _hc(plan, tensors, hip_device)
    q = _query("lower_half", D)
    x, _ = _evidence(hc, plan, B, q, seed=8, miss_seed=4)
    res = [hc.marginal_map(x, torch.from_numpy(q), return_choices=True, return_log_value=True, return_log_prob=True,
                           rows_per_chunk=r) for r in (None, 1, 7)]
    for out, ch, lv, lp in res[1:]:
        assert torch.equal(_bits(out), _bits(res[0][0]))
        assert all(torch.equal(a, b) for a, b in zip(ch, res[0][1]))
        assert torch.equal(lv, res[0][2]) and torch.equal(lp, res[0][3])


@pytest.mark.gpu
def test_gpu_marginal_map_impossible_evidence(hip_device):
    plan, tensors = _plan("cfg1_rbt8")
    D, N = plan.num_variables, 200
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
    q = np.random.default_rng(6).random(D) < 0.6
    q[var] = False
    x, masked = _evidence(hc, plan, N, q, seed=9)
    bad = torch.arange(N, device=hip_device) % 2 == 1
    x[:, var] = torch.where(bad, cc + 1, cc)  # contradicting evidence in half the rows, observed in all of them
    masked[:, var] = x[:, var]
    out, ch, lv, lp = hc.marginal_map(x, torch.from_numpy(q), return_choices=True, return_log_value=True,
                                      return_log_prob=True)
    qd = torch.from_numpy(q).to(hip_device)
    for val in (lv, lp):
        assert bool((val[bad] == -np.inf).all()) and bool(torch.isfinite(val[~bad]).all())
    assert bool((out[bad][:, qd] == -1).all())
    assert torch.equal(out[:, ~qd], masked[:, ~qd])
    assert all(bool((c[:, bad] == -1).all()) for c in ch)
    ok = ~bad
    _check_against_restatement(plan, tensors, x[ok], q, out[ok], [c[:, ok] for c in ch], lv[ok], lp[ok])


@pytest.mark.gpu
def test_gpu_marginal_map_out_of_range_evidence_is_reported_and_does_not_stick(hip_device):
    plan, tensors = _plan("cfg2_qt784")  # Categorical-256
    D, N = plan.num_variables, 64
    hc = _hc(plan, tensors, hip_device)
    q = _query("lower_half", D)
    x, masked = _evidence(hc, plan, N, q, seed=4)
    kw = dict(return_choices=True, return_log_value=True, return_log_prob=True)
    good = hc.marginal_map(x, torch.from_numpy(q), **kw)
    bad = x.clone()
    bad[5, 10] = 300  # an observed category out of range
    out, ch, lv, lp = hc.marginal_map(bad, torch.from_numpy(q), **kw)
    qd = torch.from_numpy(q).to(hip_device)
    assert bool(torch.isnan(lv[5])) and bool(torch.isnan(lp[5])) and bool((out[5, qd] == -1).all())
    assert out[5, 10] == 300 and all(bool((c[:, 5] == -1).all()) for c in ch)
    keep = torch.arange(N, device=hip_device) != 5
    assert torch.equal(out[keep], good[0][keep]) and torch.equal(lv[keep], good[2][keep])  # the other rows keep their bits
    assert torch.equal(lp[keep], good[3][keep]) and all(torch.equal(a[:, keep], b[:, keep]) for a, b in zip(ch, good[1]))
    with pytest.raises(IndexError):  # reported where hc(x) reports it, and cleared by the check
        hc.check_inputs()
    hc.check_inputs()
    again = hc.marginal_map(x, torch.from_numpy(q), **kw)
    assert torch.equal(again[0], good[0]) and torch.equal(again[2], good[2]) and torch.equal(again[3], good[3])
    assert bool(torch.isfinite(again[2]).all())
    hc.check_inputs()


@pytest.mark.gpu
def test_gpu_marginal_map_refusals(hip_device):
    plan, tensors = _case("cfg5_sos_c_k32")
    hc = _hc(plan, tensors, hip_device)
    with pytest.raises(ValueError, match="lse-sum"):
        hc.marginal_map(torch.zeros((4, plan.num_variables), dtype=torch.int64, device=hip_device), [0])
    plan, tensors = _case("cfg1_rbt8")
    D = plan.num_variables
    hc = _hc(plan, tensors, hip_device)
    x = torch.zeros((4, D), dtype=torch.int64, device=hip_device)
    with pytest.raises(ValueError, match="one query set"):
        hc.marginal_map(x, torch.ones((4, D), dtype=torch.bool))
    with pytest.raises(ValueError):
        hc.marginal_map(x, torch.ones(D + 1, dtype=torch.bool))
    with pytest.raises(ValueError):
        hc.marginal_map(x, [D])
    with pytest.raises(ValueError):
        hc.marginal_map(x[:, : D - 1], [0])
    s = hc._sampler
    assert s._key is None and s._zc is None  # refused before anything was prepared or launched
    name = plan.layers[0].params["probs"].nodes[0].config["tensor"]
    v = np.array(hc.store.export(name), dtype=np.float32)
    v[0, 0, 0] = np.nan  # a NaN input parameter: refused by prepare(), as `sample` refuses it
    hc.store.set(name, v)
    with pytest.raises(ValueError, match="NaN"):
        hc.marginal_map(x, [0])


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
def test_gpu_marginal_map_follows_training_steps(hip_device, fused):
    from cirkit_amd.training import HipTrainer

    plan, tensors, g = load_case("cfg2_qt784")
    xb = torch.from_numpy(g["x"].astype(np.int64)).to(hip_device)[:64]
    tr = HipTrainer(plan, tensors, device=hip_device, lr=0.05, fused=None if fused else False)
    assert tr.fused == fused
    q = _query("lower_half", plan.num_variables)
    miss = torch.from_numpy((np.random.default_rng(MISS_SEED).random(tuple(xb.shape)) < 0.3) & ~q).to(hip_device)
    xm = torch.where(miss, -1, xb)
    kw = dict(return_log_value=True, return_log_prob=True)
    _, lb, pb = tr.circuit.marginal_map(xm, torch.from_numpy(q), **kw)
    for _ in range(3):
        tr.step(xb)
    after, la, pa = tr.circuit.marginal_map(xm, torch.from_numpy(q), **kw)
    assert not torch.equal(lb, la) and not torch.equal(pb, pa)
    fresh, lf, pf = _hc(plan, tr.parameters(), hip_device).marginal_map(xm, torch.from_numpy(q), **kw)
    assert torch.equal(after, fresh) and torch.equal(la, lf) and torch.equal(pa, pf)
