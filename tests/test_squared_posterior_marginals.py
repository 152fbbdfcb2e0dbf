"""Posterior marginals of squared circuits for a whole set of query variables on the GPU (cirkit_amd/squared_posterior.py; the
launches: `ck_squared_down_bwd` and `ck_squared_down_leaf`, cirkit_amd/csrc/ck_sqdown.hip) against fp64 enumeration with the
repository's oracle: entry ``(b, v, s)`` of `query_log_marginals` is ``logsumexp(2 Re log c)`` over the completions of row ``b``
with ``x_v = s`` and the other query variables integrated (tests/squared_down_restatement.py; its fp64 run is pinned to the
enumeration and its fp32 run stays below a quarter of the bound asserted here: tests/test_squared_down_restatement.py, which also
recomputes the recorded expectations in tests/golden/sq_posterior_expected.npz that the larger cases here read).

Comparison (`P.check`): a state that holds at least e^-4 of its row's largest is held to ``|got - want| <= 1e-4 max(1, |want|)``
on the logarithm (`R.bound`), the others to ``S.EPS`` in linear space after the shift by the row's expected maximum; which is
which is decided from the fp64 expectation, and at most a quarter of a case's states may take the linear route.  Identities
between two GPU results use twice the bound.

Measured on an MI355X, worst error as a fraction of the bound: the tiny circuits 0.004, 32 signed units 0.006 (B = 33; no state
on the linear route), the Categorical fixture 0.002, ``log m`` of the kernels alone 0.004 and their written G 8e-7 of a block's
largest element, identities 0.004, against `state_log_marginals` 0.000 ("Posterior marginals of squared
circuits")."""
import functools

import numpy as np
import pytest
import torch

import squared_down_restatement as P
import squared_marginal_restatement as R
import squared_sampling_restatement as S
from guarded_buffers import NAN_BITS, _Guarded, _GuardedArena, _stream

pytestmark = pytest.mark.gpu


def _check(got, want, what="", factor=1.0):
    """`R.bound` on every finite value (tests/test_squared_sampling.py::_check)."""
    got = got.detach().cpu().double()
    want = torch.as_tensor(want).double()
    fin = torch.isfinite(want)
    assert bool((got[~fin] == want[~fin]).all()), f"{what}: where the expected value is not finite"
    err = (got[fin] - want[fin]).abs()
    b = factor * torch.from_numpy(R.bound(want[fin]))
    print(f"{what}: worst error {float((err / b).max()):.3f} of the bound")
    assert bool((err <= b).all()), f"{what}: {float(err.max())} against {float(b.min())}"
    return float((err / b).max())


def _kinds_read(sq):
    """The kinds of the child values the down launches of the cached plans read: slot h is read when another slot is a down fold."""
    kinds = set()
    for dp in sq._down_plans.values():
        for bt in dp.dev.values():
            for la in bt.launches:
                for row in la.host:
                    down = [int(row[2 + 3 * h]) >= 0 for h in range(la.H)]
                    kinds |= {int(row[3 + 3 * h]) for h in range(la.H) if sum(down) - down[h] > 0}
    return kinds


# ---- 1. tiny circuits ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny_expected(sum_product):
    plan, tensors, states = R.tiny_case(sum_product)
    x = P.tiny_rows()
    return plan, tensors, x, [P.expected_query_log_marginals(plan, tensors, x, q, i, states) for q, i in P.TINY_QUERIES]


@pytest.mark.parametrize("padded", [True, False], ids=["32units", "3units"])
@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_query_sets_of_the_tiny_circuits(hip_device, sum_product, padded):
    """K = 3 as it is (the shape-generic form) and padded to 32 units (the 32-unit form and its root), 5 rows."""
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, x, want = _tiny_expected(sum_product)
    if padded:
        plan, tensors = R.pad_tiny_to_32(plan, tensors, sum_product)
    sq = HipSquaredCircuit(plan, tensors, device=hip_device)
    xd = x.to(hip_device)
    for (q, i), w in zip(P.TINY_QUERIES, want):
        got, ev = sq.query_log_marginals(xd, q, i, normalized=False, return_log_evidence=True)
        assert got.shape == (5, len(q), 3) and got.dtype == torch.float32 and ev.shape == (5,)
        assert sq.last_down_launches > 0
        P.check(got, w, f"{sum_product} Q={q} I={i}")
        both = sq.log_marginal(xd, q + i, normalized=False).cpu()
        _check(torch.logsumexp(got, dim=2), both[:, None].expand(-1, len(q)), "summed over the states", factor=2.0)
        _check(ev, both, "the returned evidence", factor=2.0)
        post = sq.posterior_marginals(xd, torch.from_numpy(P.mask_of(6, q)), i)
        _check(torch.logsumexp(post, dim=2), torch.zeros(5, len(q)), "posteriors sum to one", factor=2.0)
    q, i = P.TINY_QUERIES[1]
    lz = float(sq.log_partition())
    got, ev = sq.query_log_marginals(xd, q, i, return_log_evidence=True)
    P.check(got, want[1] - lz, "normalised", factor=2.0)  # (log Z is the GPU's own)
    _check(ev, sq.log_marginal(xd, q + i).cpu(), "normalised evidence", factor=2.0)


# ---- 2. 32 signed units ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _emb32_circuit(dev, rows_per_block=1):
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, _ = R.emb32_case()
    return HipSquaredCircuit(plan, tensors, device=dev, rows_per_block=rows_per_block)


@pytest.mark.parametrize("B", [1, 3, 33])
def test_32_signed_units(hip_device, B):
    from cirkit_amd import _capi as capi

    g = P.golden()
    sq = _emb32_circuit(str(hip_device))
    xd = P.emb32_rows()[:B].to(hip_device)
    kinds, worst = set(), 0.0
    for n, (q, i) in enumerate(P.EMB32_QUERIES):
        got = sq.query_log_marginals(xd, q, i, normalized=False)
        kinds |= _kinds_read(sq)
        worst = max(worst, P.check(got, g[f"emb32_want_{n}"][:B], f"B={B} Q={q} I={i}")[0])
        one = torch.stack([sq.state_log_marginals(xd, v, sorted(set(q + i) - {v}), normalized=False) for v in sorted(q)], dim=1)
        P.check(got, one, f"B={B} Q={q} I={i} against state_log_marginals", factor=2.0, route=g[f"emb32_want_{n}"][:B])
    print(f"B={B}: worst error {worst:.3f} of the bound")
    assert kinds == {capi.CK_SQ_FULL, capi.CK_SQ_CONST, capi.CK_SQ_RANK1}


# ---- 3. a real circuit under lse-sum -----------------------------------------------------------------------------------------
def test_real_circuit_under_lse_sum(hip_device):
    """The `sq_cat_qt4x4_k5` fixture (256 states, K = 5 padded to 32 by HipCircuit): the `float` kernels, a table of logarithms."""
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, _ = R.cat_case()
    sq = HipSquaredCircuit(plan, tensors, device=hip_device)
    assert sq.c._pad_info is not None and sq.plan.layers[1].num_input_units == 32
    q, i = P.CAT_QUERY
    got = sq.query_log_marginals(P.cat_rows().to(hip_device), q, i, normalized=False)
    assert got.shape == (3, 3, 256)
    # 629 of the 2304 expected states lie below e^-4 of their row's largest, more than the linear route may take; this circuit
    # has no signed cancellation, so EVERY state is held to the bound on its logarithm (as test_squared_sampling.py holds it)
    P.check(got, P.golden()["cat_want"], f"Q={q} I={i}", min_log_share=-np.inf)


# ---- 4. the kernels alone -------------------------------------------------------------------------------------------------------
def _linear_error(got, want):
    """Worst |exp(got - max) - exp(want - max)| over (B, n) log values, max the largest expected real part of the row."""
    gr, wr = (got.real, want.real) if np.iscomplexobj(want) else (got, want)
    assert not np.isnan(gr).any()
    dead = np.isneginf(wr)
    assert bool((gr[dead] == wr[dead]).all())  # (-inf exactly)
    with np.errstate(all="ignore"):
        mx = np.where(dead, -np.inf, wr).max(axis=1, keepdims=True)
        mx = np.where(np.isfinite(mx), mx, 0.0)
        lin = lambda v, r: np.exp(r - mx) * (np.exp(1j * np.where(np.isneginf(r), 0.0, v.imag)) if np.iscomplexobj(v) else 1.0)
        return float(np.abs(lin(got, gr) - lin(want, wr)).max())


@pytest.mark.parametrize("B,R_rows", [(1, 1), (3, 2)])
@pytest.mark.parametrize("shape", list(P.LAYER_SHAPES))
@pytest.mark.parametrize("cplx", [False, True], ids=["float", "c32"])
def test_kernels_alone(hip_device, cplx, shape, B, R_rows):
    """`ck_squared_down_bwd` on a hand-built layer of two folds (`P.hand_layer_case`) and `ck_squared_down_leaf` on what it wrote,
    against the fp64 restatement of that layer.  The down arena lies between guard words with a block for EVERY child slot: the
    blocks of the children that are no down folds keep their fill, the fold's own G is left as it was.  Every written G is held
    to `S.EPS` of its row's largest element in linear space (a cancelled element of dP is accurate relative to the block, not to
    itself) and -inf exactly where the restatement has -inf; every ``log m`` to `P.check`.  With B = 3 the last row's G is all
    -inf: every child's G and every state is exactly -inf, not NaN; one weight column is 0 (a -inf row and column of dP)."""
    from cirkit_amd import _capi as capi

    assert (capi.CK_SQ_FULL, capi.CK_SQ_CONST, capi.CK_SQ_RANK1) == (P.KIND_FULL, P.KIND_CONST, P.KIND_RANK1)
    dev = hip_device
    case, Gs, lms, _, _ = P.hand_layer_case(cplx, shape, B)
    st, Ki, Ko, top, slots = P.LAYER_SHAPES[shape]
    H, n, C, e = len(slots), P.LAYER_FOLDS, P.LAYER_STATES, 2 if cplx else 1

    def words(t):
        t = t.to(torch.complex64 if cplx else torch.float32).contiguous()
        return (torch.view_as_real(t) if cplx else t).reshape(-1).float()

    sizes, fill, block_in, block_out = [], [], {}, {}
    for j, (gin, kids) in enumerate(case["folds"]):
        if gin is not None:
            block_in[j] = len(sizes)
            sizes.append(B * Ko * Ko * e)
            fill.append(words(gin))
        for h in range(H):
            block_out[(j, h)] = len(sizes)
            sizes.append(B * Ki * Ki * e)
            fill.append(torch.full((sizes[-1],), NAN_BITS, dtype=torch.int32).view(torch.float32))
    arena = _GuardedArena(sizes, dev)
    arena.fill(fill)
    host = np.zeros((n, 2 + 3 * H), dtype=np.int64)
    pools = {P.KIND_FULL: [], P.KIND_CONST: [], P.KIND_RANK1: []}
    for j, (gin, kids) in enumerate(case["folds"]):
        host[j, 0], host[j, 1] = j + 1, arena.off[block_in[j]] // e if gin is not None else -1
        for h, (dn, kd, raw, _) in enumerate(kids):
            host[j, 2 + 3 * h: 5 + 3 * h] = (arena.off[block_out[(j, h)]] // e if dn else -1, kd, sum(t.numel() for t in pools[kd]) // e)
            pools[kd].append(words(raw))
    cat = lambda ts: torch.cat(ts).to(dev) if ts else None
    full_d, cst_d, rk_d = cat(pools[P.KIND_FULL]), cat(pools[P.KIND_CONST]), cat(pools[P.KIND_RANK1])
    wd = case["w"].float().contiguous().to(dev) if st else None
    tab_d = torch.from_numpy(host).to(dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    capi.call("ck_squared_down_bwd", ptr(full_d), ptr(cst_d), ptr(rk_d), arena.ptr(), arena.words // e, host.ctypes.data, tab_d.data_ptr(), n, H,
              ptr(wd[0]) if st else None, ptr(wd[1]) if st else None, 4 if st else 0, Ki, Ko, 2 if st else 0, B, R_rows, 1 if cplx else 0,
              _stream(dev))
    downs = [(j, h) for j in range(n) for h in range(H) if slots[h][0]]
    table_d = case["table"].float().contiguous().to(dev)
    Cmax = C + 2
    vars_host = np.zeros((len(downs), 6), dtype=np.int64)
    for k, (j, h) in enumerate(downs):
        vars_host[k, :5] = (table_d[j * H + h].data_ptr(), C, Ki, case["tlog"], arena.off[block_out[(j, h)]] // e)
    vars_d = torch.from_numpy(vars_host).to(dev)
    out = _Guarded(B * len(downs) * Cmax, dev)
    capi.call("ck_squared_down_leaf", arena.ptr(), arena.words // e, vars_host.ctypes.data, vars_d.data_ptr(), len(downs), Cmax, out.out.data_ptr(),
              B, 1 if cplx else 0, _stream(dev))
    torch.cuda.synchronize(dev)
    flat = arena.read([block_out[k] for k in downs])  # (every other word -- guards, the folds' own G, the other slots -- as it was)
    bits = arena.bits.cpu()[arena.lead:]
    worst = 0.0
    for j, h in downs:
        o, sz = arena.off[block_out[(j, h)]], sizes[block_out[(j, h)]]
        assert bool((bits[o: o + sz] != NAN_BITS).all()), "a word of a down child's G was never written"
        got = flat[o: o + sz].double().numpy()
        got = (got[0::2] + 1j * got[1::2]) if cplx else got
        want = Gs[j][h].reshape(-1, Ki * Ki).expand(B, -1).numpy()
        worst = max(worst, _linear_error(got.reshape(B, Ki * Ki), want))
    print(f"{shape} B={B}: worst linear error of a written G {worst:.1e}")
    assert worst <= S.EPS
    got = out.read().double().reshape(B, len(downs), Cmax)  # (every owned word written, the guard words intact)
    assert bool(torch.isneginf(got[:, :, C:]).all())
    want = torch.stack([lms[k].expand(B, -1) for k in downs], dim=1)
    if B > 1 and not top:
        assert bool(torch.isneginf(got[B - 1, :, :C]).all()) and bool(torch.isneginf(want[B - 1]).all())
    P.check(got[:, :, :C], want, f"{shape} B={B} log m")


# ---- 5. chunks and rows per workgroup -----------------------------------------------------------------------------------------
def test_chunks_and_rows_per_block_do_not_change_a_bit(hip_device):
    sq = _emb32_circuit(str(hip_device))
    sq3 = _emb32_circuit(str(hip_device), 3)
    xd = P.emb32_rows()[:5].to(hip_device)
    for q, i in P.EMB32_QUERIES[1:]:
        ref, ev = (t.clone() for t in sq.query_log_marginals(xd, q, i, return_log_evidence=True))
        for rpc in (1, 2):
            got, ev2 = sq.query_log_marginals(xd, q, i, return_log_evidence=True, rows_per_chunk=rpc)
            assert torch.equal(got, ref) and torch.equal(ev2, ev)
        assert torch.equal(sq3.query_log_marginals(xd, q, i), ref)
        assert torch.equal(sq.posterior_marginals(xd, q, i, rows_per_chunk=2), sq3.posterior_marginals(xd, q, i))


# ---- 6. refusals and edge rows ---------------------------------------------------------------------------------------------
def test_refusals_and_edge_rows(hip_device):
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.squared import HipSquaredCircuit
    from cirkit_amd.squared_posterior import host_plan
    from cirkit_amd.templates import InputSpec, build_plan, quad_graph

    plan, tensors, x = R.gauss_case()
    gs = HipSquaredCircuit(plan, tensors, device=hip_device)
    xg = x[:2].to(torch.float32).to(hip_device)
    for call in (lambda: gs.query_log_marginals(xg, [1, 2]), lambda: gs.posterior_marginals(xg, [1], [3])):
        with pytest.raises(NotImplementedError, match="Gaussian"):
            call()
    assert not gs._down_plans and getattr(gs, "_down_buf", None) is None  # (nothing was planned or allocated)
    dag = build_plan(quad_graph(4, 4), input_layer=InputSpec("embedding", 3), sum_product="cp", num_input_units=4, num_sum_units=4,
                     sum_activation="none", semiring="complex-lse-sum")
    with pytest.raises(NotImplementedError):  # (refused by the constructor, as before; and its ancestries are no paths)
        HipSquaredCircuit(dag, init_plan_tensors(dag, seed=3), device=hip_device)
    with pytest.raises(NotImplementedError, match="DAG"):
        host_plan(dag, [5, 6], P.mask_of(16, [5, 6]))
    sq = _emb32_circuit(str(hip_device))
    xd = P.emb32_rows()[:4].to(hip_device)
    with pytest.raises(ValueError, match="integrated out"):
        sq.query_log_marginals(xd, [3, 4], [4, 5])
    with pytest.raises(ValueError, match="at least one"):
        sq.query_log_marginals(xd, [])
    with pytest.raises(ValueError, match="ONE scope"):
        sq.query_log_marginals(xd, [1], torch.zeros((2, 16), dtype=torch.bool))
    with pytest.raises(ValueError, match="ONE scope"):
        sq.posterior_marginals(xd, torch.ones((2, 16), dtype=torch.bool))
    q, i = [0, 5, 6], [1]
    ref, ev = (t.clone() for t in sq.query_log_marginals(xd, q, i, return_log_evidence=True))
    bad = xd.clone()
    bad[1, 9] = -1  # observed
    bad[2, 1] = -7  # integrated: ignored
    bad[3, 5] = -2  # a query variable: ignored
    got, ev2 = sq.query_log_marginals(bad, q, i, return_log_evidence=True)
    assert bool(torch.isnan(got[1]).all()) and bool(torch.isnan(ev2[1])) and torch.equal(got[[0, 2, 3]], ref[[0, 2, 3]])
    assert torch.equal(ev2[[0, 2, 3]], ev[[0, 2, 3]])
    assert torch.equal(sq.query_log_marginals(xd, q, i), ref)  # a later valid call is unaffected
    everything = list(range(16))
    got, ev = sq.query_log_marginals(xd, everything, normalized=False, return_log_evidence=True)
    lz = sq.log_partition().cpu().expand(4)
    _check(ev, lz, "nothing observed: the evidence is Z", factor=2.0)
    _check(torch.logsumexp(got, dim=2), lz[:, None].expand(-1, 16), "nothing observed: every variable sums to Z", factor=2.0)
    assert torch.equal(got[0], got[3])  # (no entry of x is read)
