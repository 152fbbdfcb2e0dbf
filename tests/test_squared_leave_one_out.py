"""Leave-one-out conditionals of squared circuits on the GPU (cirkit_amd/squared_loo.py; the launches: `ck_squared_loo_down` and
`ck_squared_loo_leaf`, cirkit_amd/csrc/ck_sqloo.hip) against fp64 enumeration with the repository's oracle: entry ``(b, v, s)`` of
`leave_one_out_log_marginals` is ``2 Re log c`` of row ``b`` with ``x_v = s`` (tests/squared_loo_restatement.py; its fp64 run is
pinned to the enumeration and its fp32 run stays below half of the bounds asserted here: tests/test_squared_loo_restatement.py).

Comparison (`P.check`, `L.check_entries`): a state that holds at least e^-4 of its row's largest is held to
``|got - want| <= 1e-4 max(1, |want|)`` on the logarithm (`R.bound`), the others to ``S.EPS`` in linear space after the shift by the
row's expected maximum; which is which is decided from the fp64 expectation, and at most a quarter of a case's states (entries) may
take the linear route.  The Categorical fixture has no signed cancellation: every state is held to the bound on its logarithm.
Identities between two GPU results use twice the bound.

Measured on an MI355X, worst error as a fraction of the bound (unnormalised table / normalised over the states / per entry): 32
signed units at B = 33 0.044 / 0.389 / 0.389 with 190 of 1584 states on the linear route (worst linear error 1.5e-6), the tiny
circuits 0.021 at most, the Categorical fixture 0.002 / 0.051 / 0.032, the kernels alone 0.040 on their three leaf modes and 7.4e-7 of a row's
largest element on a written D; the observed state against `log_prob` 0.021 and `conditional_log_probs` against
`conditional_log_prob` 0.019 of twice the bound ("Leave-one-out conditionals of squared circuits")."""
import functools

import numpy as np
import pytest
import torch

import squared_down_restatement as P
import squared_loo_restatement as L
import squared_marginal_restatement as R
import squared_sampling_restatement as S
from guarded_buffers import NAN_BITS, _Guarded, _GuardedArena, _stream

pytestmark = pytest.mark.gpu


def _check(got, want, what="", factor=1.0):
    """`R.bound` on every finite value (tests/test_squared_sampling.py::_check)."""
    got = got.detach().cpu().double()
    want = torch.as_tensor(want).detach().cpu().double()
    fin = torch.isfinite(want)
    assert bool((got[~fin] == want[~fin]).all()), f"{what}: where the expected value is not finite"
    err = (got[fin] - want[fin]).abs()
    b = factor * torch.from_numpy(R.bound(want[fin]))
    print(f"{what}: worst error {float((err / b).max()):.3f} of the bound")
    assert bool((err <= b).all()), f"{what}: {float(err.max())} against {float(b.min())}"


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case and its expectation for ALL variables, computed once (a query set is a selection of its Q axis)."""
    plan, tensors, states, rows, queries, share = L.cases()[name]
    return plan, tensors, states, rows, queries, share, L.expected_loo_log_marginals(plan, tensors, rows, range(plan.num_variables), states)


@functools.lru_cache(maxsize=None)
def _circuit(name, dev):
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors = _case(name)[:2]
    return HipSquaredCircuit(plan, tensors, device=dev)


def _three_methods(sq, name, x, want, queries, share, dev):
    """All three methods against the enumeration `want` (B, D, C) for the rows `x`."""
    B, D = x.shape
    xd = x.to(dev)
    for q in queries:
        raw = sq.leave_one_out_log_marginals(xd, q, normalized=False)
        assert raw.shape == (B, len(q), want.shape[2]) and raw.dtype == torch.float32 and sq.last_loo_launches > 1
        P.check(raw, want[:, q], f"{name} B={B} Q={q} unnormalised", min_log_share=share)
        post = sq.leave_one_out(xd, torch.from_numpy(P.mask_of(D, q)))
        P.check(post, L.normalise(want[:, q]), f"{name} B={B} Q={q} normalised", min_log_share=share)
        _check(torch.logsumexp(post, dim=2), torch.zeros(B, len(q)), "conditionals sum to one", factor=2.0)
    allv = list(range(D))
    clp = sq.conditional_log_probs(xd)
    assert clp.shape == (B, D) and clp.dtype == torch.float32
    L.check_entries(clp, L.entries(L.normalise(want), x, allv), f"{name} B={B} conditional_log_probs", share)
    return clp


# ---- 1. tiny circuits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("units", [32, 3], ids=["32units", "3units"])
@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_tiny_circuits(hip_device, sum_product, units):
    """K = 3 as it is (the VALU form and its root) and padded to 32 units (the register-tile form, its 32 -> 1 root and the -inf
    derivatives the zero weights of the padding give), the Hadamard form in `cp`; 5 rows."""
    name = f"tiny-{sum_product}-{units}"
    plan, tensors, states, x, queries, share, want = _case(name)
    sq = _circuit(name, str(hip_device))
    xd = x.to(hip_device)
    clp = _three_methods(sq, name, x, want, queries, share, hip_device)
    raw = sq.leave_one_out_log_marginals(xd, normalized=False)
    lp = sq.log_prob(xd) + sq.log_partition()
    _check(L.entries(raw, x, range(6)), lp[:, None].expand(-1, 6).cpu(), "the observed state is 2 Re log c", factor=2.0)
    _check(sq.leave_one_out_log_marginals(xd, [0, 1, 4]), raw[:, [0, 1, 4]].cpu() - float(sq.log_partition()), "normalised", factor=2.0)
    for v in (0, 3, 5):
        _check(clp[:, v], sq.conditional_log_prob(xd, [v]).cpu(), f"conditional_log_prob of variable {v}", factor=2.0)


# ---- 2. 32 signed units ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 33])
def test_32_signed_units(hip_device, B):
    """One full row tile plus one row at B = 33; the register-tile form with siblings, Hadamard layers, the 32 -> 1 root."""
    plan, tensors, states, x, queries, share, want = _case("emb32")
    sq = _circuit("emb32", str(hip_device))
    _three_methods(sq, "emb32", x[:B], want[:B], queries, share, hip_device)
    lp = sq.log_prob(x[:B].to(hip_device))
    got = sq.leave_one_out_log_marginals(x[:B].to(hip_device))
    _check(L.entries(got, x[:B], range(16)), lp[:, None].expand(-1, 16).cpu(), "the observed state is log_prob", factor=2.0)


# ---- 3. a real circuit under lse-sum -----------------------------------------------------------------------------------------
def test_real_circuit_under_lse_sum(hip_device):
    """The `sq_cat_qt4x4_k5` fixture (256 states, K = 5 padded to 32 by HipCircuit): the `float` kernels, a table of logarithms."""
    plan, tensors, states, x, queries, share, want = _case("cat")
    sq = _circuit("cat", str(hip_device))
    assert sq.c._pad_info is not None and sq.plan.layers[1].num_input_units == 32
    _three_methods(sq, "cat", x, want, queries[:1], share, hip_device)


# ---- 4. the kernels alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 35])
@pytest.mark.parametrize("shape", list(L.LAYER_SHAPES))
@pytest.mark.parametrize("cplx", [False, True], ids=["float", "c32"])
def test_kernels_alone(hip_device, cplx, shape, B):
    """`ck_squared_loo_down` on a hand-built layer of two folds (`L.hand_layer`) and `ck_squared_loo_leaf`, in its three modes, on
    what it wrote, against the fp64 restatement of that layer.  Both arenas lie between guard words, the derivative arena with a
    block for EVERY child slot: the block of a child that is no down fold keeps its fill, the fold's own D is left as it was.  Every
    written D is held to `S.EPS` of its row's largest element in linear space, its sign included, and is -inf exactly where the
    restatement has -inf: the unit behind the zero weight column (a linear sum that is exactly 0) in every row and, with B = 35,
    the whole last row (an all -inf derivative: every state -inf too, NaN once normalised)."""
    from cirkit_amd import _capi as capi

    dev = hip_device
    case = L.hand_layer(cplx, shape, B)
    Ds, lms = L.hand_layer_run(case)
    wt, Ki, Ko, top, slots = L.LAYER_SHAPES[shape]
    H, n, C, e = len(slots), L.LAYER_FOLDS, L.LAYER_STATES, 2 if cplx else 1

    def words(t):
        t = t.to(torch.complex64 if cplx else torch.float32).contiguous()
        return (torch.view_as_real(t) if cplx else t).reshape(-1).float()

    sizes, fill, block_in, block_out = [], [], {}, {}
    vsizes, vfill = [], []
    for j, (din, kids) in enumerate(case["folds"]):
        if din is not None:
            block_in[j] = len(sizes)
            sizes.append(B * Ko * e)
            fill.append(words(din))
        for h in range(H):
            block_out[(j, h)] = len(sizes)
            sizes.append(B * Ki * e)
            fill.append(torch.full((sizes[-1],), NAN_BITS, dtype=torch.int32).view(torch.float32))
            vsizes.append(B * Ki * e)
            vfill.append(words(kids[h]))
    arena = _GuardedArena(sizes, dev)
    arena.fill(fill)
    vals = _GuardedArena(vsizes, dev)
    vals.fill(vfill)
    host = np.zeros((n, 2 + 2 * H), dtype=np.int64)
    for j in range(n):
        host[j, 0], host[j, 1] = j + 1, arena.off[block_in[j]] // e if j in block_in else -1
        for h, dn in enumerate(slots):
            host[j, 2 + 2 * h: 4 + 2 * h] = (arena.off[block_out[(j, h)]] // e if dn else -1, vals.off[j * H + h] // e)
    wd = case["w"].float().contiguous().to(dev) if wt else None
    tab_d = torch.from_numpy(host).to(dev)
    capi.call("ck_squared_loo_down", vals.ptr(), vals.words // e, arena.ptr(), arena.words // e, host.ctypes.data, tab_d.data_ptr(), n, H,
              wd.data_ptr() if wt else None, 4 if wt else 0, Ki, Ko, B, 1 if cplx else 0, 0, _stream(dev))
    downs = [(j, h) for j in range(n) for h in range(H) if slots[h]]
    table_d = case["table"].float().contiguous().to(dev)
    xd = case["x"].to(dev)
    Cmax = C + 2
    vars_host = np.zeros((len(downs), 6), dtype=np.int64)
    for k, (j, h) in enumerate(downs):
        vars_host[k] = (table_d[j * H + h].data_ptr(), C, Ki, case["tlog"], arena.off[block_out[(j, h)]] // e, j * H + h)
    vars_d = torch.from_numpy(vars_host).to(dev)
    outs = []
    for mode in (capi.CK_SQ_LOO_TABLE, capi.CK_SQ_LOO_NORMALISED, capi.CK_SQ_LOO_ENTRY):
        out = _Guarded(B * len(downs) * (1 if mode == capi.CK_SQ_LOO_ENTRY else Cmax), dev)
        capi.call("ck_squared_loo_leaf", arena.ptr(), arena.words // e, vars_host.ctypes.data, vars_d.data_ptr(), len(downs), Cmax, xd.data_ptr(),
                  int(xd.shape[1]), out.out.data_ptr(), mode, B, 1 if cplx else 0, _stream(dev))
        outs.append(out)
    torch.cuda.synchronize(dev)
    vals.read([])  # (c's arena: not a word changed)
    flat = arena.read([block_out[k] for k in downs])  # (every other word -- guards, the folds' own D, the other slots -- as it was)
    bits = arena.bits.cpu()[arena.lead:]
    worst = 0.0
    for j, h in downs:
        o, sz = arena.off[block_out[(j, h)]], sizes[block_out[(j, h)]]
        assert bool((bits[o: o + sz] != NAN_BITS).all()), "a word of a down child's D was never written"
        got = flat[o: o + sz].double().numpy()
        got = (got[0::2] + 1j * got[1::2]) if cplx else got
        want = Ds[j][h].expand(B, -1).numpy()
        if wt:
            assert bool(np.isneginf(want.real[:, -1]).all())  # (the linear sum that is exactly 0)
        worst = max(worst, L.linear_error(got.reshape(B, Ki), want))
    print(f"{shape} B={B}: worst linear error of a written D {worst:.1e}")
    assert worst <= S.EPS
    want = torch.stack([lms[k].expand(B, -1) for k in downs], dim=1)
    dead = B > 1 and not top
    live = slice(0, B - 1) if dead else slice(0, B)
    got = outs[0].read().double().reshape(B, len(downs), Cmax)  # (every owned word written, the guard words intact)
    assert bool(torch.isneginf(got[:, :, C:]).all())
    if dead:
        assert bool(torch.isneginf(got[B - 1, :, :C]).all()) and bool(torch.isneginf(want[B - 1]).all())
    P.check(got[:, :, :C], want, f"{shape} B={B} log m")
    norm = outs[1].read().double().reshape(B, len(downs), Cmax)
    assert bool(torch.isneginf(norm[live, :, C:]).all())
    P.check(norm[live, :, :C], L.normalise(want[live]), f"{shape} B={B} normalised")
    ent = outs[2].read().double().reshape(B, len(downs))
    xs = case["x"][:, [j * H + h for j, h in downs]]
    L.check_entries(ent[live], torch.gather(L.normalise(want[live]), 2, xs[live, :, None])[:, :, 0], f"{shape} B={B} per entry")
    if dead:  # (no leave-one-out mass: NaN)
        assert bool(torch.isnan(norm[B - 1, :, :C]).all()) and bool(torch.isnan(ent[B - 1]).all())


def test_forced_valu_form_agrees(hip_device):
    """`form` 1 of `ck_squared_loo_down` (what scripts/bench_squared_loo.py times beside the register-tile form) on 32 units."""
    from cirkit_amd.squared_loo import leave_one_out_log_marginals

    sq = _circuit("emb32", str(hip_device))
    x, want = _case("emb32")[3][:33], _case("emb32")[6][:33]
    got = leave_one_out_log_marginals(sq, x.to(hip_device), None, normalized=False, form=1)
    P.check(got, want, "the VALU form on 32 units")


# ---- 5. chunks --------------------------------------------------------------------------------------------------------------
def test_chunks_do_not_change_a_bit(hip_device):
    sq = _circuit("emb32", str(hip_device))
    xd = _case("emb32")[3][:33].to(hip_device)
    B = int(xd.shape[0])
    q = [1, 6, 11, 12]
    ref = [sq.leave_one_out_log_marginals(xd, q).clone(), sq.leave_one_out(xd).clone(), sq.conditional_log_probs(xd).clone()]
    for rpc in (1, 7, B):
        got = [sq.leave_one_out_log_marginals(xd, q, rows_per_chunk=rpc), sq.leave_one_out(xd, rows_per_chunk=rpc),
               sq.conditional_log_probs(xd, rows_per_chunk=rpc)]
        for g, r in zip(got, ref):
            assert torch.equal(g, r), f"rows_per_chunk={rpc}"
    with pytest.raises(ValueError, match="positive"):
        sq.leave_one_out(xd, rows_per_chunk=0)


# ---- 6. refusals, edge rows, launch counts ------------------------------------------------------------------------------------
def test_refusals_edge_rows_and_launch_counts(hip_device):
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, x = R.gauss_case()
    gs = HipSquaredCircuit(plan, tensors, device=hip_device)
    xg = x[:2].to(torch.float32).to(hip_device)
    for call in (lambda: gs.leave_one_out_log_marginals(xg, [1, 2]), lambda: gs.leave_one_out(xg), lambda: gs.conditional_log_probs(xg)):
        with pytest.raises(NotImplementedError, match="Gaussian"):
            call()
    assert not gs._loo_plans and gs._loo_buf is None  # (nothing was planned or allocated)
    with pytest.raises(NotImplementedError, match="complex parameter"):
        t = dict(_case("tiny-cp-3")[1])
        k = next(iter(t))
        t[k] = np.asarray(t[k]).astype(np.complex64)
        HipSquaredCircuit(_case("tiny-cp-3")[0], t, device=hip_device)
    sq = _circuit("emb32", str(hip_device))
    xd = _case("emb32")[3][:4].to(hip_device)
    with pytest.raises(ValueError, match="at least one"):
        sq.leave_one_out_log_marginals(xd, [])
    with pytest.raises(ValueError, match="at least one"):
        sq.leave_one_out(xd, torch.zeros(16, dtype=torch.bool))
    with pytest.raises(ValueError, match="subset"):
        sq.leave_one_out(xd, [16])
    with pytest.raises(ValueError, match="expected x of shape"):
        sq.conditional_log_probs(xd[:, :5])
    q = [0, 5, 6]
    ref = [sq.leave_one_out_log_marginals(xd, q).clone(), sq.leave_one_out(xd, q).clone(), sq.conditional_log_probs(xd).clone()]
    bad = xd.clone()
    bad[1, 9] = -1  # beside the query variables
    bad[3, 5] = -2  # a query variable: it is evidence for the others
    got = [sq.leave_one_out_log_marginals(bad, q), sq.leave_one_out(bad, q), sq.conditional_log_probs(bad)]
    for g, r in zip(got, ref):
        assert bool(torch.isnan(g[[1, 3]]).all()) and torch.equal(g[[0, 2]], r[[0, 2]])
    assert torch.equal(sq.leave_one_out(xd, q), ref[1])  # a later valid call is unaffected
    # the launches: one per layer of c with a fold above Q, and the leaves; the same for every Q of a tree that reaches the root
    layers_above = lambda qs: len({p for p, f in P.down_folds(sq.plan, qs) if sq.plan.layers[p].inputs is not None})
    for qs in ([3], q, list(range(16))):
        sq.leave_one_out(xd, qs)
        assert sq.last_loo_launches == layers_above(qs) + 1
        sq.leave_one_out(xd, qs, rows_per_chunk=3)
        assert sq.last_loo_launches == 2 * (layers_above(qs) + 1)
    sq.conditional_log_probs(xd)
    assert sq.last_loo_launches == layers_above(range(16)) + 1
    assert 3 <= len(sq._loo_plans) <= 8 and sq._loo_buf is not None
