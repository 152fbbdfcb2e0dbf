"""Autoregressive conditionals and coding on the GPU (`HipCircuit.autoregressive_conditionals`, `autoregressive_log_probs`,
`coding_tables`, cirkit_amd/autoregressive.py, cirkit_amd/codec.py, cirkit_amd/csrc/ck_ar.hip; DESIGN.md section 11,
"Autoregressive conditionals and coding").

Every entry is compared with the fp64 restatement (tests/autoregressive_restatement.py, pinned on the CPU by
tests/test_autoregressive_restatement.py) under the rule of tests/test_leave_one_out.py: the yardstick is the SAME restatement
run in float32 on the test's own plan and evidence; the GPU must be within 4 x that error, at least 1e-6 -- absolute on
probabilities and log probabilities, relative to 1 + |moment| for Gaussian moments -- and the same rule bounds |sum_c p - 1|.
Nothing in a bound comes from what the GPU returns.  One reference of 5 rows per plan serves the batches of 1, 3 and 5 rows:
at 5 rows there are 80 to 180 expanded rows, more than one 32-row tile and not a multiple of 32, and 7 rows per chunk cut
through a row's block.  Measured yardsticks and GPU errors: DESIGN.md section 11.
"""
import functools

import numpy as np
import pytest
import torch

from autoregressive_restatement import autoregressive_restated, covered, expand, log_prob_restated, quantise
from test_autoregressive_restatement import adversarial_rows
from test_leave_one_out import _err, _evidence, _gauss, _to_dev
from test_leave_one_out import _plan as _loo_plan
from test_mpe import _hc
from test_posterior_marginals import _states

DISCRETE = ["kat_bernoulli_f0o0", "kat_bernoulli_f1o1", "quadtree_4x4_kron_k3", "plan_quadgraph_1x4x4_cp",
            "quadgraph_6x6_tucker_k4", "binomial_qg6x6_k4", "qt2_cp_k32", "qt2_cpt_k64", "cat256_k32"]
PLANS = DISCRETE + ["pd_gauss_6x6_k4", "plan_clt_mixed6_cp"]
ROWS = (1, 3, 5)
CFG2_POSITIONS = [0, 1, 391, 392, 783]


@functools.lru_cache(maxsize=None)
def _plan(name):
    if name == "cat256_k32":  # the 4 x 4 Categorical-256, K = 32 image circuit of tests/test_interval.py
        from test_interval import _templated

        return _templated(name)
    return _loo_plan(name)


def _order(plan, kind):
    cov = covered(plan)
    if kind == "ascending":
        return None
    return cov[::-1] if kind == "reversed" else [int(v) for v in np.random.default_rng(61).permutation(cov)]


@functools.lru_cache(maxsize=None)
def _reference(name, order_kind="ascending", positions=None, B=ROWS[-1]):
    """(x, fp64 result, fp64 log p(x), bounds): computed once, shared, never written to."""
    plan, tensors = _plan(name)
    x = _evidence(plan, B, 60)
    pos = None if positions is None else list(positions)
    r64 = autoregressive_restated(plan, tensors, x, _order(plan, order_kind), pos)
    r32 = autoregressive_restated(plan, tensors, x, _order(plan, order_kind), pos, dtype=np.float32)
    g = _gauss(plan)
    yard = {"logp": _err(r32["logp"], r64["logp"], False)}
    if r64["p"] is not None:
        yard["p"] = _err(r32["p"], r64["p"], g)
        yard["sum"] = 0.0 if g else float(np.abs(r32["p"].astype(np.float64).sum(2) - 1).max())
    print(f"  {name} / {order_kind}: fp32-restatement yardsticks " + ", ".join(f"{k} {v:.3e}" for k, v in yard.items()))
    return x, r64, log_prob_restated(plan, tensors, x), {k: max(4 * v, 1e-6) for k, v in yard.items()}


def _check(hc, plan, x, want, logpx, bound, order=None, positions=None, what=""):
    """Test 1 on the rows `x`: both queries against the fp64 restatement, the row sums, the chain rule."""
    g, B = _gauss(plan), x.shape[0]
    xb = _to_dev(plan, x, hc.device)
    lp = hc.autoregressive_log_probs(xb, order, positions=positions)
    P = want["logp"].shape[1]
    assert tuple(lp.shape) == (B, P) and lp.dtype == torch.float32 and lp.device.type == "cuda"
    lpn = lp.cpu().numpy()
    el = _err(lpn, want["logp"][:B], False)
    print(f"  {what}B={B}: GPU error log p {el:.3e} (bound {bound['logp']:.3e})")
    assert el <= bound["logp"], (B, el, bound["logp"])
    assert (lpn[want["missing"][:B]] == 0).all()
    if positions is None:
        chain = float(np.abs(lpn.astype(np.float64).sum(1) - logpx[:B]).max())
        print(f"  {what}B={B}: |sum_i log p - log p(x)| {chain:.3e} (bound {P * bound['logp']:.3e})")
        assert chain <= P * bound["logp"]
    if want["p"] is None:
        with pytest.raises(NotImplementedError):
            hc.autoregressive_conditionals(xb, order, positions=positions)
        return
    p = hc.autoregressive_conditionals(xb, order, positions=positions)
    assert tuple(p.shape) == (B,) + want["p"].shape[1:] and p.dtype == torch.float32 and p.device.type == "cuda"
    pn = p.cpu().numpy()
    e = _err(pn, want["p"][:B], g)
    print(f"  {what}B={B}: GPU error p {e:.3e} (bound {bound['p']:.3e})")
    assert e <= bound["p"], (B, e, bound["p"])
    if not g:
        s = float(np.abs(pn.astype(np.float64).sum(2) - 1).max())
        print(f"  {what}B={B}: |sum_c p - 1| {s:.3e} (bound {bound['sum']:.3e})")
        assert s <= bound["sum"], (B, s, bound["sum"])
        states = _states(plan)
        for j, i in enumerate(want["positions"]):  # padding: states past a variable's own count are exactly 0
            assert (pn[:, j, int(states[want["order"][i]]) :] == 0).all()


# ------------------------------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("name", PLANS)
def test_gpu_autoregressive_equals_restatement(hip_device, name):
    plan, tensors = _plan(name)
    x, want, logpx, bound = _reference(name)
    hc = _hc(plan, tensors, hip_device)
    for B in ROWS:
        _check(hc, plan, x[:B], want, logpx, bound)


@pytest.mark.gpu
def test_gpu_flagship_circuit_at_five_steps(hip_device):
    plan, tensors = _plan("cfg2_qt784")
    x, want, logpx, bound = _reference("cfg2_qt784", "ascending", tuple(CFG2_POSITIONS), 1)
    hc = _hc(plan, tensors, hip_device)
    _check(hc, plan, x, want, logpx, bound, None, CFG2_POSITIONS)
    xb = _to_dev(plan, x, hip_device)
    t = hc.coding_tables(xb, positions=CFG2_POSITIONS)
    p = hc.autoregressive_conditionals(xb, positions=CFG2_POSITIONS)
    assert np.array_equal(t.cpu().numpy()[0], quantise(p.cpu().numpy()[0], np.full(5, 256), 16))


# ------------------------------------------------------------------------------------- 2. against the path already trusted
@pytest.mark.gpu
@pytest.mark.parametrize("name", PLANS)
def test_gpu_equals_leave_one_out_on_the_host_expanded_batch(hip_device, name):
    """The conditionals are bit for bit the diagonal of `leave_one_out` on the batch expanded on the host.  The log
    probabilities need not be: the expanded row hides the value at order[i] from the evidence forward, so `ck_ar_log_probs`
    reads the unit's log value from a log table of its own (log of the stored probabilities, the Gaussian density formed in
    place) where `conditional_log_probs` reads what the forward's input kernels wrote; both are held to the bound of test 1
    against the same fp64 numbers, their difference to twice that bound."""
    plan, tensors = _plan(name)
    x, want, _, bound = _reference(name)
    hc = _hc(plan, tensors, hip_device)
    xb = _to_dev(plan, x, hip_device)
    order = want["order"]
    rows = torch.arange(x.shape[0] * len(order), device=hip_device)
    var = torch.tensor(order * x.shape[0], device=hip_device)
    if want["p"] is not None:
        xe, mask, _, _ = expand(plan, x)
        got = hc.leave_one_out(_to_dev(plan, np.where(mask, 0, xe), hip_device), None, torch.from_numpy(mask).to(hip_device))
        cov = covered(plan)
        qi = torch.tensor([cov.index(v) for v in order] * x.shape[0], device=hip_device)
        p = hc.autoregressive_conditionals(xb)
        assert torch.equal(p.reshape(got.shape[0], -1), got[rows, qi])
    xe, mask, _, _ = expand(plan, x, keep_own=True)
    loo = hc.conditional_log_probs(_to_dev(plan, np.where(mask, 0, xe), hip_device), torch.from_numpy(mask).to(hip_device))
    loo = loo[rows, var].reshape(x.shape[0], -1).cpu().numpy()
    lp = hc.autoregressive_log_probs(xb).cpu().numpy()
    assert _err(loo, want["logp"], False) <= bound["logp"]
    d = _err(lp, loo, False)
    print(f"  {name}: |autoregressive_log_probs - conditional_log_probs| {d:.3e} (bound {2 * bound['logp']:.3e})")
    assert d <= 2 * bound["logp"]


# ------------------------------------------------------------------------------------------------ 3. independence and layout
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["quadtree_4x4_kron_k3", "qt2_cpt_k64", "pd_gauss_6x6_k4", "cat256_k32"])
def test_gpu_later_steps_do_not_influence_a_row(hip_device, name):
    plan, tensors = _plan(name)
    x, want, _, _ = _reference(name)
    hc = _hc(plan, tensors, hip_device)
    order, g = want["order"], _gauss(plan)
    xb = _to_dev(plan, x, hip_device)
    p, lp = hc.autoregressive_conditionals(xb).clone(), hc.autoregressive_log_probs(xb).clone()
    t = None if g else hc.coding_tables(xb).clone()
    other = _evidence(plan, x.shape[0], 62)
    for i in (0, 1, len(order) // 2, len(order) - 1):
        for fill in ("random", "sentinel"):
            x2 = x.copy()
            later = order[i:]
            x2[:, later] = other[:, later] if fill == "random" else (np.nan if g else -1)
            x2b = _to_dev(plan, x2, hip_device)
            assert torch.equal(hc.autoregressive_conditionals(x2b, positions=[i]), p[:, i : i + 1]), (i, fill)
            if t is not None:
                assert torch.equal(hc.coding_tables(x2b, positions=[i]), t[:, i : i + 1]), (i, fill)
            x2[:, order[i]] = x[:, order[i]]  # (the log probability reads the row's own value at step i, nothing later)
            assert torch.equal(hc.autoregressive_log_probs(_to_dev(plan, x2, hip_device), positions=[i]), lp[:, i : i + 1])
    xs = x.copy()
    xs[:, order[2]] = np.nan if g else -1  # a sentinel of the caller's: log prob exactly 0 there, missing at every later step
    got = hc.autoregressive_log_probs(_to_dev(plan, xs, hip_device))
    assert bool((got[:, 2] == 0).all()) and torch.equal(got[:, :2], lp[:, :2]) and not torch.equal(got[:, 3:], lp[:, 3:])


@pytest.mark.gpu
@pytest.mark.parametrize("order_kind", ["reversed", "permuted"])
@pytest.mark.parametrize("name", ["quadgraph_6x6_tucker_k4", "qt2_cp_k32", "pd_gauss_6x6_k4", "plan_clt_mixed6_cp"])
def test_gpu_other_orders_equal_restatement(hip_device, name, order_kind):
    plan, tensors = _plan(name)
    x, want, logpx, bound = _reference(name, order_kind)
    hc = _hc(plan, tensors, hip_device)
    _check(hc, plan, x, want, logpx, bound, _order(plan, order_kind), None, f"{order_kind} ")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["binomial_qg6x6_k4", "qt2_cp_k32", "pd_gauss_6x6_k4"])
def test_gpu_positions_chunkings_and_repeated_calls(hip_device, name):
    plan, tensors = _plan(name)
    x, want, _, _ = _reference(name)
    hc = _hc(plan, tensors, hip_device)
    g, n = _gauss(plan), len(want["order"])
    xb = _to_dev(plan, x, hip_device)
    order = _order(plan, "permuted")
    calls = [lambda **kw: hc.autoregressive_conditionals(xb, order, **kw), lambda **kw: hc.autoregressive_log_probs(xb, order, **kw)]
    if not g:
        calls.append(lambda **kw: hc.coding_tables(xb, order, precision=12, **kw))
    for call in calls:
        full = call().clone()
        for r in (None, 7, 32, 1):
            assert torch.equal(call(rows_per_chunk=r), full), r
        sub = sorted({0, n // 2 - 1, n // 2, n - 1})
        assert torch.equal(call(positions=sub), full[:, sub])
        assert torch.equal(call(positions=sub[::-1] + sub, rows_per_chunk=7), full[:, sub])
        assert torch.equal(call(positions=range(3, 9)), full[:, 3:9])
        m = torch.zeros(n, dtype=torch.bool)
        m[sub] = True
        assert torch.equal(call(positions=m), full[:, sub])
        assert torch.equal(call(positions=[n - 1]), full[:, n - 1 :])
    with pytest.raises(ValueError):
        hc.autoregressive_conditionals(xb, order[:-1])
    with pytest.raises(ValueError):
        hc.autoregressive_log_probs(xb, positions=[n])
    with pytest.raises(ValueError):
        hc.autoregressive_log_probs(xb, rows_per_chunk=0)
    if not g:
        with pytest.raises(ValueError):
            hc.coding_tables(xb, precision=7)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["qt2_cp_k32", "quadgraph_6x6_tucker_k4", "pd_gauss_6x6_k4"])
def test_gpu_outputs_stay_inside_their_buffers(hip_device, name):
    from cirkit_amd.autoregressive import _ar
    from guarded_buffers import _Guarded

    plan, tensors = _plan(name)
    x, _, _, _ = _reference(name)
    hc = _hc(plan, tensors, hip_device)
    xb = _to_dev(plan, x, hip_device)
    g = _gauss(plan)
    want = hc.autoregressive_conditionals(xb), hc.autoregressive_log_probs(xb), None if g else hc.coding_tables(xb)
    st = _ar(hc)
    ps, s = st.ps, st.ps.s
    ids, steps, gauss = st.check(None, None, "autoregressive_conditionals")
    N, C = x.shape[0] * len(steps), int(want[0].shape[2])
    gp, gl, gv = _Guarded(N * C, hip_device), _Guarded(N, hip_device, lead=1), _Guarded(N, hip_device, lead=3)
    gt = _Guarded(N * (C + 1), hip_device, lead=1)
    ge = _Guarded(N * s.D * (1 if g else 2), hip_device)  # (the expanded evidence: fp32, or int64 as pairs of words)
    with torch.cuda.device(hip_device):
        stream = torch.cuda.current_stream(hip_device).cuda_stream
        xm = s.evidence_batch(xb, [])
        st.param_tables()
        order_pos, pos = st.order_tables(ids, steps)
        bad = torch.zeros(N, dtype=torch.int32, device=hip_device)
        rowobs = torch.empty(N, dtype=xm.dtype, device=hip_device)
        rowvar = gv.out.view(torch.int32)
        xe = ge.out.view(xm.dtype).view(N, s.D)
        st.expand(xm, order_pos, pos, 0, N, rowvar, rowobs, bad, stream, xe=xe)
        bd = ps.evidence_forward(xe, bad, stream)
        der = st.loo.down.run(bd, stream)
        st.leaves(bd, der, gauss, C, rowvar, bad, gp.out, stream)
        st.log_probs(bd, der, rowvar, rowobs, bad, gl.out, stream)
        if not g:
            st.quantise(gp.out, rowvar, N, C, 16, gt.out.view(torch.int32), stream)
        torch.cuda.synchronize()
    assert np.array_equal(gp.read().numpy().reshape(want[0].shape), want[0].cpu().numpy(), equal_nan=True)
    assert np.array_equal(gl.read().numpy().reshape(want[1].shape), want[1].cpu().numpy(), equal_nan=True)
    assert np.array_equal(gv.raw().numpy(), np.tile(np.asarray(ids, dtype=np.int32), x.shape[0]))
    ge.raw()
    if not g:
        assert np.array_equal(gt.raw().numpy().reshape(want[2].shape), want[2].cpu().numpy())


@pytest.mark.gpu
def test_gpu_store_writes_invalidate_the_tables(hip_device):
    plan, tensors = _loo_plan("cfg1_rbt8")
    x = _evidence(plan, 3, 63)
    hc = _hc(plan, tensors, hip_device)
    xb = _to_dev(plan, x, hip_device)
    before = hc.autoregressive_conditionals(xb).clone(), hc.autoregressive_log_probs(xb).clone(), hc.coding_tables(xb).clone()
    rng = np.random.default_rng(64)
    changed = dict(tensors)
    for l in (plan.layers[0], plan.layers[2]):  # the Categorical tables and a sum weight
        for gph in l.params.values():
            n = gph.nodes[0].config["tensor"]
            changed[n] = (np.asarray(tensors[n]) + rng.normal(size=np.asarray(tensors[n]).shape)).astype(np.float32)
            hc.store.set(n, changed[n])
    after = hc.autoregressive_conditionals(xb), hc.autoregressive_log_probs(xb), hc.coding_tables(xb)
    assert all(not torch.equal(a, b) for a, b in zip(after, before))
    want = autoregressive_restated(plan, changed, x)
    w32 = autoregressive_restated(plan, changed, x, dtype=np.float32)
    assert _err(after[0].cpu().numpy(), want["p"], False) <= max(4 * _err(w32["p"], want["p"], False), 1e-6)
    fresh = _hc(plan, changed, hip_device)
    assert torch.equal(fresh.autoregressive_conditionals(xb), after[0]) and torch.equal(fresh.coding_tables(xb), after[2])


# ------------------------------------------------------------------------------------------ 4. stepwise against all-at-once
@pytest.mark.gpu
@pytest.mark.parametrize("name", DISCRETE)
def test_gpu_stepwise_tables_equal_the_all_steps_call(hip_device, name):
    """What keeps ``compress(..., batched=True)``: step i alone, on the B rows, gives column i of the one all-steps call."""
    plan, tensors = _plan(name)
    x, want, _, _ = _reference(name)
    hc = _hc(plan, tensors, hip_device)
    xb = _to_dev(plan, x, hip_device)
    full = hc.coding_tables(xb).clone()
    C = int(_states(plan)[want["order"]].max())
    assert tuple(full.shape) == (x.shape[0], len(want["order"]), C + 1) and full.dtype == torch.int32
    assert bool((full[..., 0] == 0).all()) and bool((full[..., -1] == 1 << 16).all())
    for i in range(len(want["order"])):
        assert torch.equal(hc.coding_tables(xb, positions=[i]), full[:, i : i + 1]), i
        held = x.copy()
        held[:, want["order"][i:]] = -1  # (what the decoder holds at step i)
        assert torch.equal(hc.coding_tables(_to_dev(plan, held, hip_device), positions=[i]), full[:, i : i + 1]), i


# ---------------------------------------------------------------------------------------------------------- 5. the quantiser
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["kat_bernoulli_f1o1", "binomial_qg6x6_k4", "qt2_cpt_k64", "cat256_k32"])
def test_gpu_quantiser_equals_numpy_on_the_gpus_conditionals(hip_device, name):
    plan, tensors = _plan(name)
    x, want, _, _ = _reference(name)
    hc = _hc(plan, tensors, hip_device)
    xb = _to_dev(plan, x, hip_device)
    p = hc.autoregressive_conditionals(xb).cpu().numpy()
    ns = np.tile(_states(plan)[want["order"]], x.shape[0])
    for precision in (10 if p.shape[2] <= 256 else 12, 16, 24):
        t = hc.coding_tables(xb, precision=precision).cpu().numpy()
        assert np.array_equal(t.reshape(-1, t.shape[2]), quantise(p.reshape(-1, p.shape[2]), ns, precision)), precision


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [10, 12, 16, 24])
def test_gpu_quantiser_equals_numpy_on_adversarial_rows(hip_device, precision):
    from cirkit_amd import _capi as capi

    p, ns = adversarial_rows()
    rng = np.random.default_rng(65)
    more = rng.dirichlet(np.full(256, 0.2), size=70).astype(np.float32)  # more rows than one workgroup's four waves
    p, ns = np.concatenate([p, more]), np.concatenate([ns, np.full(70, 256)])
    rows, C = p.shape
    with torch.cuda.device(hip_device):
        pd = torch.from_numpy(p).to(hip_device)
        rowvar = torch.arange(rows, dtype=torch.int32, device=hip_device)
        states = torch.from_numpy(ns.astype(np.int32)).to(hip_device)
        out = torch.full((rows, C + 1), -7, dtype=torch.int32, device=hip_device)
        capi.call("ck_ar_quantise", pd.data_ptr(), rowvar.data_ptr(), states.data_ptr(), rows, C, precision, out.data_ptr(),
                  torch.cuda.current_stream(hip_device).cuda_stream)
        torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), quantise(p, ns, precision))


# --------------------------------------------------------------------------------------------------- 6. the codec on the device
@pytest.mark.gpu
@pytest.mark.parametrize("name", DISCRETE)
def test_gpu_codec_round_trip(hip_device, name):
    from cirkit_amd import codec

    plan, tensors = _plan(name)
    x, want, logpx, _ = _reference(name)
    hc = _hc(plan, tensors, hip_device)
    xi = torch.from_numpy(x.astype(np.int64))
    for batched in (False, True):
        blobs, counts = codec.compress(hc, xi, batched=batched, return_counts=True)
        assert len(blobs) == x.shape[0]
        back = codec.decompress(hc, blobs)
        assert back.dtype == torch.int64 and torch.equal(back, xi), batched
        bits = np.array([8 * len(b) for b in blobs])
        ideal = codec.ideal_bits(counts, 16)
        assert (bits <= ideal + codec.OVERHEAD_BITS).all()
    gap = ideal + logpx / np.log(2)  # quantised ideal minus -log2 p(x)
    xb = _to_dev(plan, x, hip_device)
    fwd = hc(xb)[:, 0, 0].cpu().numpy().astype(np.float64)  # (read before the next forward reuses the arena)
    fwd = -(fwd - hc(xb, integrate_vars=list(range(plan.num_variables)))[:, 0, 0].cpu().numpy().astype(np.float64)) / np.log(2)
    D = len(want["order"])
    print(f"  {name}: {bits.mean() / D:.4f} coded, {ideal.mean() / D:.4f} quantised ideal, {fwd.mean() / D:.4f} -log2 p(x) from "
          f"forward, bits per variable; quantised ideal minus -log2 p(x) {(ideal - fwd).mean():.4f} bits per row "
          f"(restatement: {gap.mean():.4f})")
    order = _order(plan, "permuted")
    assert torch.equal(codec.decompress(hc, codec.compress(hc, xi, order, precision=12), order, precision=12), xi)
    bad = bytearray(blobs[0])
    bad[9 if len(bad) > 9 else 3] ^= 0x10
    try:
        got = codec.decompress(hc, [bytes(bad)] + blobs[1:])
        assert not torch.equal(got[0], xi[0]) and torch.equal(got[1:], xi[1:])
    except ValueError:
        pass
    with pytest.raises(ValueError):
        codec.compress(hc, torch.full_like(xi, -1))
    with pytest.raises(ValueError):
        codec.compress(hc, xi, precision=25)


# ------------------------------------------------------------------------------------------------- 7. out-of-range evidence
@pytest.mark.gpu
@pytest.mark.parametrize("at", [3, 12])
def test_gpu_out_of_range_evidence_is_that_rows_nan_and_the_flag(hip_device, at):
    plan, tensors = _plan("qt2_cp_k32")
    x, _, _, _ = _reference("qt2_cp_k32")
    hc = _hc(plan, tensors, hip_device)
    xb = _to_dev(plan, x, hip_device)
    good = hc.autoregressive_conditionals(xb).clone(), hc.autoregressive_log_probs(xb).clone(), hc.coding_tables(xb).clone()
    hc.check_inputs()
    bad = xb.clone()
    S = int(_states(plan)[at])
    bad[2, at] = S + 44
    keep = torch.arange(xb.shape[0], device=hip_device) != 2
    uniform = torch.from_numpy(quantise(np.full((1, good[0].shape[2]), np.nan, dtype=np.float32), np.array([S]), 16)[0]).to(hip_device)
    for r in (None, 7):
        for positions in (None, [0, 1]):  # (steps before the bad variable's too: the whole row is refused)
            cols = slice(None) if positions is None else positions
            p = hc.autoregressive_conditionals(bad, positions=positions, rows_per_chunk=r)
            with pytest.raises(IndexError):
                hc.check_inputs()
            lp = hc.autoregressive_log_probs(bad, positions=positions, rows_per_chunk=r)
            t = hc.coding_tables(bad, positions=positions, rows_per_chunk=r)
            assert bool(torch.isnan(p[2]).all()) and bool(torch.isnan(lp[2]).all())
            assert bool((t[2] == uniform).all())
            assert torch.equal(p[keep], good[0][keep][:, cols]) and torch.equal(lp[keep], good[1][keep][:, cols])
            assert torch.equal(t[keep], good[2][keep][:, cols])
            with pytest.raises(IndexError):
                hc.check_inputs()
            hc.check_inputs()
    assert torch.equal(hc.autoregressive_conditionals(xb), good[0])
    hc.check_inputs()
