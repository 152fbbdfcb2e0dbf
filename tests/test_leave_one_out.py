"""Leave-one-out conditionals on the GPU (`HipCircuit.leave_one_out`, `HipCircuit.conditional_log_probs`,
cirkit_amd/leave_one_out.py, cirkit_amd/csrc/ck_loo.hip; DESIGN.md section 11, "Leave-one-out conditionals").

Every entry is compared with the fp64 restatement (tests/loo_restatement.py, pinned on the CPU by
tests/test_loo_restatement.py).  Tolerance: the project's rule (tests/test_posterior_marginals.py) -- the yardstick is the SAME
restatement run in float32 against its fp64 run on the test's own plan and evidence; the GPU must be within 4 x that error,
at least 1e-6: absolute on probabilities and log probabilities, relative to 1 + |moment| for Gaussian moments.  The same
rule bounds |sum_c p - 1| by 4 x the fp32 restatement's own row-sum error.  Nothing in a bound comes from what the GPU
returns.  One reference of 70 rows per (plan, missing pattern) serves the batches of 1, 31, 33 and 70 rows (rows are
independent, 32 is the row tile of the matrix-core paths).  Measured yardsticks and GPU errors: DESIGN.md section 11.
"""
import functools

import numpy as np
import pytest
import torch

from loo_restatement import leave_one_out_restated
from test_loo_restatement import KAT, any_case, zero_case
from test_expected_statistics import SMALL
from test_mpe import _case, _hc
from test_posterior_marginals import _states

GPU_PLANS = list(SMALL) + ["qg_cp_k3"] + KAT + ["quadtree_4x4_kron_k3", "plan_quadgraph_1x4x4_cp", "quadgraph_6x6_tucker_k4",
                                                "binomial_qg6x6_k4", "pd_gauss_6x6_k4", "cfg1_rbt8"]
ROWS = (1, 31, 33, 70)
MISSING = ("none", "lower_half", "per_row")


def _gauss(plan) -> bool:
    return any(l.type == "gaussian" for l in plan.layers)


def _plan(name):
    """The plan with the tensors as the device holds them (fp32 values; the restatement reads the same numbers)."""
    plan, tensors = any_case(name)
    return plan, {k: np.asarray(v, dtype=np.float32) if np.asarray(v).dtype.kind == "f" else v for k, v in tensors.items()}


def _evidence(plan, B, seed) -> np.ndarray:
    """Random cells: every observed value is as likely wrong as right, which is what the query is for."""
    rng = np.random.default_rng(seed)
    c = _states(plan)
    x = rng.normal(size=(B, plan.num_variables))
    d = c > 0
    x[:, d] = rng.integers(0, c[d], size=(B, int(d.sum())))
    return x


def _missing(kind, B, D):
    if kind == "none":
        return None
    if kind == "lower_half":
        return np.arange(D) >= D // 2
    return np.random.default_rng(31).random((B, D)) < 0.3


def _to_dev(plan, x, dev):
    return torch.from_numpy(x.astype(np.float32) if _gauss(plan) else x.astype(np.int64)).to(dev)


def _mask_dev(m, dev):
    return None if m is None else torch.from_numpy(m).to(dev)


def _err(got, want, gauss) -> float:
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    same = (np.isnan(got) == np.isnan(want)) & ((got == -np.inf) == (want == -np.inf))
    assert same.all(), "NaN / -inf entries differ from the restatement's"
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    d = np.abs(got[fin] - want[fin])
    return float((d / (1 + np.abs(want[fin]))).max() if gauss else d.max())


@functools.lru_cache(maxsize=None)
def _reference(name, missing_kind):
    """(x, missing, fp64 result, bounds) of 70 rows: computed once, shared, never written to."""
    plan, tensors = _plan(name)
    B, D = ROWS[-1], plan.num_variables
    x = _evidence(plan, B, 30)
    miss = _missing(missing_kind, B, D)
    r64 = leave_one_out_restated(plan, tensors, x, None, miss)
    r32 = leave_one_out_restated(plan, tensors, x, None, miss, dtype=np.float32)
    g = _gauss(plan)
    yard = {"p": _err(r32["p"], r64["p"], g), "logp": _err(r32["logp"], r64["logp"], False),
            "sum": 0.0 if g else float(np.abs(r32["p"].astype(np.float64).sum(2) - 1).max())}
    print(f"  {name} / {missing_kind}: fp32-restatement yardsticks " + ", ".join(f"{k} {v:.3e}" for k, v in yard.items()))
    return x, miss, r64, {k: max(4 * v, 1e-6) for k, v in yard.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("missing_kind", MISSING)
@pytest.mark.parametrize("name", GPU_PLANS)
def test_gpu_leave_one_out_equals_restatement(hip_device, name, missing_kind):
    plan, tensors = _plan(name)
    D, g = plan.num_variables, _gauss(plan)
    x, miss, want, bound = _reference(name, missing_kind)
    hc = _hc(plan, tensors, hip_device)
    states = _states(plan)
    for B in ROWS:
        xb, mb = _to_dev(plan, x[:B], hip_device), _mask_dev(miss if miss is None or miss.ndim == 1 else miss[:B], hip_device)
        p = hc.leave_one_out(xb, None, mb)
        lp = hc.conditional_log_probs(xb, mb)
        torch.cuda.synchronize()
        assert tuple(p.shape) == (B,) + want["p"].shape[1:] and p.dtype == torch.float32 and p.device.type == "cuda"
        assert tuple(lp.shape) == (B, D) and lp.dtype == torch.float32
        pn, lpn = p.cpu().numpy(), lp.cpu().numpy()
        e, el = _err(pn, want["p"][:B], g), _err(lpn, want["logp"][:B], False)
        print(f"  B={B}: GPU error p {e:.3e} (bound {bound['p']:.3e}), log p {el:.3e} (bound {bound['logp']:.3e})")
        assert e <= bound["p"], (B, e, bound["p"])
        assert el <= bound["logp"], (B, el, bound["logp"])
        assert (lpn[want["mask"][:B]] == 0).all()  # exactly 0 where the row misses the variable
        if not g:
            s = float(np.abs(pn.astype(np.float64).sum(2) - 1).max())
            print(f"  B={B}: |sum_c p - 1| {s:.3e} (bound {bound['sum']:.3e})")
            assert s <= bound["sum"], (B, s, bound["sum"])
            for q, v in enumerate(want["query"]):  # padding: states past a variable's own count are exactly 0
                assert (pn[:, q, int(states[v]) :] == 0).all()
            # log p(x_v | rest) is the log of the gathered entry
            obs = ~want["mask"][:B]
            xi = np.where(obs, x[:B], 0).astype(np.int64)
            gathered = np.take_along_axis(pn.astype(np.float64), xi[:, :, None], axis=2)[:, :, 0]
            big = obs & (gathered > 1e-3)
            assert np.abs(np.log(gathered[big]) - lpn[big]).max() <= bound["logp"] + bound["p"] / 1e-3
    # query sets: one variable, a mix of observed and missing variables, as ids, a range and a mask
    xb, mb = _to_dev(plan, x, hip_device), _mask_dev(miss, hip_device)
    full = hc.leave_one_out(xb, None, mb)
    mix = sorted({0, D // 2 - 1, D // 2, D - 1})
    assert torch.equal(hc.leave_one_out(xb, [D - 1], mb), full[:, D - 1 :])
    assert torch.equal(hc.leave_one_out(xb, mix, mb), full[:, mix])
    assert torch.equal(hc.leave_one_out(xb, range(D), mb), full)
    qm = torch.zeros(D, dtype=torch.bool)
    qm[mix] = True
    assert torch.equal(hc.leave_one_out(xb, qm, mb), full[:, mix])
    # a query variable's own value does not matter
    xs = xb.clone()
    xs[:, mix[0]] = 0
    assert torch.equal(hc.leave_one_out(xs, [mix[0]], mb), full[:, mix[:1]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["qt2_cp_k32", "qg_cp_k3", "quadgraph_6x6_tucker_k4", "binomial_qg6x6_k4", "pd_gauss_6x6_k4"])
def test_gpu_missing_query_variables_give_the_posterior_marginals(hip_device, name):
    from posterior_restatement import posterior_restated
    from test_posterior_marginals import _bound as posterior_bound

    plan, tensors = _plan(name)
    D = plan.num_variables
    x, _, want, bound = _reference(name, "lower_half")
    query = list(range(D // 2, D))
    hc = _hc(plan, tensors, hip_device)
    xb = _to_dev(plan, x, hip_device)
    loo = hc.leave_one_out(xb, query, query).cpu().numpy()
    post = hc.posterior_marginals(xb, query).cpu().numpy()
    xm = x.copy()
    xm[:, query] = np.nan if _gauss(plan) else -1
    pb, _ = posterior_bound(plan, tensors, xm, query, posterior_restated(plan, tensors, xm, query)["p"])
    e = _err(loo, post, _gauss(plan))
    print(f"  |leave_one_out - posterior_marginals| {e:.3e} (bounds {bound['p']:.3e} + {pb:.3e})")
    assert e <= bound["p"] + pb


@pytest.mark.gpu
def test_gpu_conditional_log_probs_accepts_mixed_scopes(hip_device):
    plan, tensors = _plan("plan_clt_mixed6_cp")  # Categorical over the even variables, Gaussian over the odd ones
    B, D = 33, plan.num_variables
    x = _evidence(plan, B, 32)
    miss = np.random.default_rng(33).random((B, D)) < 0.25
    want = leave_one_out_restated(plan, tensors, x, [0], miss)
    w32 = leave_one_out_restated(plan, tensors, x, [0], miss, dtype=np.float32)
    bound = max(4 * _err(w32["logp"], want["logp"], False), 1e-6)
    hc = _hc(plan, tensors, hip_device)
    xb = torch.from_numpy(x.astype(np.float32)).to(hip_device)
    lp = hc.conditional_log_probs(xb, torch.from_numpy(miss).to(hip_device)).cpu().numpy()
    e = _err(lp, want["logp"], False)
    print(f"  GPU error log p {e:.3e} (bound {bound:.3e})")
    assert e <= bound and (lp[want["mask"]] == 0).all()
    with pytest.raises(NotImplementedError):
        hc.leave_one_out(xb)  # (the default query set mixes the kinds)
    assert tuple(hc.leave_one_out(xb, [0, 2]).shape) == (B, 2, 3) and tuple(hc.leave_one_out(xb, [1]).shape) == (B, 1, 2)


@pytest.mark.gpu
def test_gpu_zero_cases_sit_where_the_restatement_puts_them(hip_device):
    plan, tensors, x, tname = zero_case()
    D = plan.num_variables
    clean_plan, clean = _case("kat_bernoulli_f1o1")
    hc = _hc(clean_plan, clean, hip_device)
    xb = _to_dev(plan, x, hip_device)
    before = hc.leave_one_out(xb).clone()
    hc.store.set(tname, np.asarray(tensors[tname], dtype=np.float32))  # (the zeros go in through the store)
    want = leave_one_out_restated(plan, tensors, x, list(range(D)))
    w32 = leave_one_out_restated(plan, tensors, x, list(range(D)), dtype=np.float32)
    assert want["zero_share"][0, 1] > 0.1 and want["logev"][1] == -np.inf
    p, lp = hc.leave_one_out(xb).cpu().numpy(), hc.conditional_log_probs(xb).cpu().numpy()
    assert np.isnan(p[1, 1:]).all() and np.array_equal(p[1, 0], [1.0, 0.0])  # no mass / a proper distribution
    assert np.isnan(lp[1, 1:]).all() and lp[1, 0] == -np.inf
    e, el = _err(p, want["p"], False), _err(lp, want["logp"], False)  # (NaN and -inf in the restatement's places)
    assert e <= max(4 * _err(w32["p"], want["p"], False), 1e-6), e
    assert el <= max(4 * _err(w32["logp"], want["logp"], False), 1e-6), el
    assert not torch.equal(before.cpu(), torch.from_numpy(p))


@pytest.mark.gpu
def test_gpu_out_of_range_evidence_is_that_rows_nan_and_the_flag(hip_device):
    plan, tensors = _plan("qt2_cp_k32")
    x, _, want, bound = _reference("qt2_cp_k32", "none")
    hc = _hc(plan, tensors, hip_device)
    xb = _to_dev(plan, x, hip_device)
    good = hc.leave_one_out(xb), hc.conditional_log_probs(xb)
    hc.check_inputs()
    bad = xb.clone()
    bad[5, 3] = int(_states(plan)[3]) + 44
    keep = torch.arange(xb.shape[0], device=hip_device) != 5
    for r in (None, 1, 7):
        p, lp = hc.leave_one_out(bad, rows_per_chunk=r), hc.conditional_log_probs(bad, rows_per_chunk=r)
        assert bool(torch.isnan(p[5]).all()) and bool(torch.isnan(lp[5]).all())
        assert torch.equal(p[keep], good[0][keep]) and torch.equal(lp[keep], good[1][keep])
        with pytest.raises(IndexError):
            hc.check_inputs()
        hc.check_inputs()
    assert torch.equal(hc.leave_one_out(xb), good[0])
    hc.check_inputs()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["qt2_cpt_k64", "qg_cp_k32", "qt2_tucker_k32", "quadtree_4x4_kron_k3", "pd_gauss_6x6_k4"])
def test_gpu_results_are_bit_identical_across_calls_and_chunkings(hip_device, name):
    plan, tensors = _plan(name)
    x, miss, _, _ = _reference(name, "per_row")
    hc = _hc(plan, tensors, hip_device)
    xb, mb = _to_dev(plan, x, hip_device), _mask_dev(miss, hip_device)
    first = hc.leave_one_out(xb, None, mb).clone(), hc.conditional_log_probs(xb, mb).clone()
    for r in (None, None, 1, 7):
        p, lp = hc.leave_one_out(xb, None, mb, rows_per_chunk=r), hc.conditional_log_probs(xb, mb, rows_per_chunk=r)
        assert torch.equal(p, first[0]) and torch.equal(lp, first[1]), r


@pytest.mark.gpu
def test_gpu_store_writes_invalidate_the_tables(hip_device):
    plan, tensors = _plan("cfg1_rbt8")
    x, _, _, _ = _reference("cfg1_rbt8", "none")
    hc = _hc(plan, tensors, hip_device)
    xb = _to_dev(plan, x, hip_device)
    before = hc.leave_one_out(xb).clone(), hc.conditional_log_probs(xb).clone()
    rng = np.random.default_rng(34)
    changed = dict(tensors)
    for l in (plan.layers[0], plan.layers[2]):  # the Categorical tables and a sum weight
        for gph in l.params.values():
            n = gph.nodes[0].config["tensor"]
            changed[n] = (np.asarray(tensors[n]) + rng.normal(size=np.asarray(tensors[n]).shape)).astype(np.float32)
            hc.store.set(n, changed[n])
    p, lp = hc.leave_one_out(xb), hc.conditional_log_probs(xb)
    assert not torch.equal(p, before[0]) and not torch.equal(lp, before[1])
    want = leave_one_out_restated(plan, changed, x)
    w32 = leave_one_out_restated(plan, changed, x, dtype=np.float32)
    assert _err(p.cpu().numpy(), want["p"], False) <= max(4 * _err(w32["p"], want["p"], False), 1e-6)
    fresh = _hc(plan, changed, hip_device)
    assert torch.equal(fresh.leave_one_out(xb), p) and torch.equal(fresh.conditional_log_probs(xb), lp)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["qt2_cp_k32", "qg_cp_k3", "pd_gauss_6x6_k4"])
def test_gpu_outputs_stay_inside_their_buffers(hip_device, name):
    from cirkit_amd.leave_one_out import _loo
    from test_em_training import _Guarded

    plan, tensors = _plan(name)
    x, _, _, _ = _reference(name, "none")
    B = 33
    hc = _hc(plan, tensors, hip_device)
    xb = _to_dev(plan, x[:B], hip_device)
    want = hc.leave_one_out(xb), hc.conditional_log_probs(xb)
    st = _loo(hc)
    ps, s = st.ps, st.ps.s
    ids = st.covered
    gauss = st.check_query(ids)
    q = st.query_tables(ids, gauss)
    gp = _Guarded(np.zeros(tuple(want[0].shape), dtype=np.float32), hip_device)
    gl = _Guarded(np.zeros(tuple(want[1].shape), dtype=np.float32), hip_device)
    with torch.cuda.device(hip_device):
        stream = torch.cuda.current_stream(hip_device).cuda_stream
        xm = s.evidence_batch(xb, [])
        bad = torch.zeros(B, dtype=torch.int32, device=hip_device)
        bd = ps.evidence_forward(xm, bad, stream)
        der = st.derivative_pass(bd, stream)
        st.leaves(bd, der, q, gauss, bad, gp.out, stream)
        st.log_probs(bd, der, xm, bad, gl.out, stream)
        torch.cuda.synchronize()
    assert np.array_equal(gp.read(), want[0].cpu().numpy(), equal_nan=True)
    assert np.array_equal(gl.read(), want[1].cpu().numpy(), equal_nan=True)
