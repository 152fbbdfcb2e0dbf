"""Exact sampling and all-state conditionals of squared circuits on the GPU (cirkit_amd/squared_sampling.py; the path launch:
`ck_squared_path_bwd`, cirkit_amd/csrc/ck_sqpath.hip) against fp64 enumeration with the repository's oracle: column ``s`` of
`state_log_marginals` is ``logsumexp(2 Re log c)`` over the completions of the row with ``x_v = s``
(tests/squared_sampling_restatement.py; its fp32 run stays below a quarter of the bound asserted here and its fp64 run is pinned
to the enumeration: tests/test_squared_sampling_restatement.py, which also checks the recorded expectations in
tests/golden/sq_sampling_expected.npz that the larger cases here read instead of enumerating again).

Bound: ``|got - want| <= 1e-4 max(1, |want|)`` on the log value (`R.bound`); identities between two GPU results use twice
that.  Draws are compared one by one with the fp64 restated sampler: a row may differ only where one of its uniforms lies within
4 EPS of a boundary of its bin (`S.near_rows`), and the samplers' distributions are tested by chi-square against enumeration."""
import functools

import numpy as np
import pytest
import torch

import squared_marginal_restatement as R
import squared_sampling_restatement as S
from guarded_buffers import _Guarded, _stream

pytestmark = pytest.mark.gpu


def _check(got, want, what="", factor=1.0):
    got = got.detach().cpu().double()
    want = torch.as_tensor(want).double()
    fin = torch.isfinite(want)
    assert bool((got[~fin] == want[~fin]).all()), f"{what}: where the expected value is not finite"
    err = (got[fin] - want[fin]).abs()
    b = factor * torch.from_numpy(R.bound(want[fin]))
    print(f"{what}: worst error {float((err / b).max()):.3f} of the bound")
    assert bool((err <= b).all()), f"{what}: {float(err.max())} against {float(b.min())}"
    return float((err / b).max())


def _chi2_p(counts, expected):
    """tests/test_sampling.py::_chi2_p: cells with tiny expectations merged into one."""
    scipy_stats = pytest.importorskip("scipy.stats")
    keep = expected >= 5
    obs = np.append(counts[keep], counts[~keep].sum())
    exp = np.append(expected[keep], expected[~keep].sum())
    if exp[-1] == 0:
        obs, exp = obs[:-1], exp[:-1]
    exp = exp * obs.sum() / exp.sum()
    return float(scipy_stats.chisquare(obs, exp).pvalue)


# ---- 1. tiny circuits ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny_expected(sum_product):
    plan, tensors, states = R.tiny_case(sum_product)
    x = R.rows_of(6, states, 5, seed=S.TINY_ROWS_SEED)
    return plan, tensors, x, [S.enumerated_state_log_marginals(plan, tensors, x, v, m, states) for v, m in S.tiny_queries()]


@pytest.mark.parametrize("padded", [True, False], ids=["32units", "3units"])
@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_every_variable_of_the_tiny_circuits(hip_device, sum_product, padded):
    """K = 3 as it is (the shape-generic form) and padded to 32 units (the 32-unit form and its root), 5 rows, every variable
    with 8 masks of the others."""
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, x, want = _tiny_expected(sum_product)
    if padded:
        plan, tensors = R.pad_tiny_to_32(plan, tensors, sum_product)
    sq = HipSquaredCircuit(plan, tensors, device=hip_device)
    xd = x.to(hip_device)
    for (v, m), w in zip(S.tiny_queries(), want):
        ids = np.nonzero(m)[0].tolist()
        got = sq.state_log_marginals(xd, v, ids, normalized=False)
        assert got.shape == (5, 3) and got.dtype == torch.float32
        _check(got, w, f"v={v} M={ids}")
        both = sq.log_marginal(xd, ids + [v], normalized=False)
        _check(torch.logsumexp(got, dim=1), both.cpu(), "summed over the states", factor=2.0)
        _check(torch.logsumexp(sq.posterior(xd, v, ids), dim=1), torch.zeros(5), "posterior sums to one", factor=2.0)
    v, m = S.tiny_queries()[9]
    _check(sq.state_log_marginals(xd, v, torch.from_numpy(m)), want[9] - float(sq.log_partition()), "normalised", factor=2.0)


# ---- 2. 32 signed units ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _emb32_circuit(dev, rows_per_block=1):
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, _ = R.emb32_case()
    return HipSquaredCircuit(plan, tensors, device=dev, rows_per_block=rows_per_block)


def _kinds_read(sq):
    """The sibling kinds on the level tables the path launches of the cached plans read."""
    from cirkit_amd.squared_sampling import sampler

    kinds = set()
    for op in sampler(sq).orders.values():
        for tb in op.dev.values():
            for row in tb.host.reshape(-1, tb.host.shape[-1]):
                kinds |= {int(k) for k in row[8: 8 + 2 * int(row[6]): 2]}
    return kinds


@pytest.mark.parametrize("B", [1, 3, 33])
def test_32_signed_units(hip_device, B):
    from cirkit_amd import _capi as capi

    g = S.golden()
    sq = _emb32_circuit(str(hip_device))
    xd = torch.from_numpy(g["emb32_x"])[:B].to(hip_device)
    kinds, worst = set(), 0.0
    for (v, m), w in zip(S.emb32_queries(), g["emb32_want"]):
        got = sq.state_log_marginals(xd, v, torch.from_numpy(m), normalized=False)
        kinds |= _kinds_read(sq)
        worst = max(worst, _check(got, w[:B], f"B={B} v={v} M={np.nonzero(m)[0].tolist()}"))
    print(f"B={B}: worst error {worst:.3f} of the bound")
    assert kinds == {capi.CK_SQ_FULL, capi.CK_SQ_CONST, capi.CK_SQ_RANK1}
    sq.state_log_marginals(xd, 0, [])
    assert sq.last_mixed_launches == 0  # everything else observed: c's forward and the path launch
    sq.state_log_marginals(xd, 0, [15, 5])
    assert sq.last_mixed_launches > 0  # scattered missing pixels: mixed siblings


def test_chunks_and_rows_per_block_do_not_change_a_bit(hip_device):
    g = S.golden()
    sq = _emb32_circuit(str(hip_device))
    sq3 = _emb32_circuit(str(hip_device), 3)
    xd = torch.from_numpy(g["emb32_x"])[:5].to(hip_device)
    for v, m in S.emb32_queries()[2::5]:
        ref = sq.state_log_marginals(xd, v, torch.from_numpy(m)).clone()
        for rpc in (1, 2):
            assert torch.equal(sq.state_log_marginals(xd, v, torch.from_numpy(m), rows_per_chunk=rpc), ref)
        assert torch.equal(sq3.state_log_marginals(xd, v, torch.from_numpy(m)), ref)


# ---- 3. a real circuit under lse-sum -----------------------------------------------------------------------------------------
def test_real_circuit_under_lse_sum(hip_device):
    """The `sq_cat_qt4x4_k5` fixture (256 states, K = 5 padded to 32 by HipCircuit): the `float` kernels, a table of logarithms."""
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, states = R.cat_case()
    x = torch.from_numpy(np.random.default_rng(S.CAT_ROWS_SEED).integers(0, states, size=(3, 16)))
    sq = HipSquaredCircuit(plan, tensors, device=hip_device)
    assert sq.c._pad_info is not None and sq.plan.layers[1].num_input_units == 32
    for (v, m), w in zip(S.cat_queries(), S.golden()["cat_want"]):
        got = sq.state_log_marginals(x.to(hip_device), v, torch.from_numpy(m), normalized=False)
        assert got.shape == (3, 256)
        _check(got, w, f"v={v} M={np.nonzero(m)[0].tolist()}")


# ---- 4. the kernel alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,R_rows", [(1, 1), (3, 2)])
@pytest.mark.parametrize("shape", list(S.PATH_SHAPES))
@pytest.mark.parametrize("cplx", [False, True], ids=["float", "c32"])
def test_kernel_alone(hip_device, cplx, shape, B, R_rows):
    """`ck_squared_path_bwd` on a hand-built path (`S.hand_path_case`) against the fp64 restatement of that path, held to
    `R.bound` on every ``log m_b(s)``: the data are chosen so that every state holds at least e^-4 of its row's largest (the
    states the bound can be asked of; the fp32 restatement stays below 0.002 of it, tests/test_squared_sampling_restatement.py).
    The siblings take the three kinds in turn; with B = 3 the last row of every RANK-1 sibling is all -inf (the gradient is
    -inf everywhere: every state is exactly -inf, not NaN) and one weight column of the last staged level is 0 (a -inf row
    and column of dP).  ``log m`` lies between guard words; the draw lands in its column alone."""
    from cirkit_amd import _capi as capi

    assert (capi.CK_SQ_FULL, capi.CK_SQ_CONST, capi.CK_SQ_RANK1) == (S.KIND_FULL, S.KIND_CONST, S.KIND_RANK1)
    dev = hip_device
    (levels, table, tlog), want, _, _ = S.hand_path_case(cplx, shape, B)
    K, C = S.PATH_SHAPES[shape][1], S.PATH_STATES
    e = 2 if cplx else 1

    def words(t):
        t = t.to(torch.complex64 if cplx else torch.float32).contiguous()
        return (torch.view_as_real(t) if cplx else t).reshape(-1).float()

    S_max = max(1, max(len(sibs) for _, _, _, _, sibs in levels))
    host = np.zeros((len(levels), 8 + 2 * S_max), dtype=np.int64)
    pools = {S.KIND_FULL: [], S.KIND_CONST: [], S.KIND_RANK1: []}
    keep = []
    for li, (st, Ki, Ko, w, sibs) in enumerate(levels):
        if st:
            wd = w.float().contiguous().to(dev)
            keep.append(wd)
            host[li, 0], host[li, 1], host[li, 4], host[li, 5] = capi.CK_SQ_PATH_STAGES, 1, wd[0].data_ptr(), wd[1].data_ptr()
        host[li, 2], host[li, 3], host[li, 6] = Ki, Ko if st else Ki, len(sibs)
        for h, (kd, raw, _) in enumerate(sibs):
            host[li, 8 + 2 * h], host[li, 9 + 2 * h] = kd, sum(t.numel() for t in pools[kd]) // e
            pools[kd].append(words(raw))
    cat = lambda ts: torch.cat(ts).to(dev) if ts else None
    full_d, cst_d, rk_d = cat(pools[S.KIND_FULL]), cat(pools[S.KIND_CONST]), cat(pools[S.KIND_RANK1])
    table_d, lev_d = table.float().contiguous().to(dev), torch.from_numpy(host).to(dev)
    out = _Guarded(B * C, dev)
    D, var = 5, 3
    x = torch.full((B, D), 7, dtype=torch.int64, device=dev)
    x_out = torch.full((B, D), 7, dtype=torch.int64, device=dev)
    dead = torch.zeros(B, dtype=torch.int32, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    capi.call("ck_squared_path_bwd", ptr(full_d), ptr(cst_d), ptr(rk_d), host.ctypes.data, lev_d.data_ptr(), len(levels), S_max,
              table_d.data_ptr(), 1, C, K, tlog, out.out.data_ptr(), x.data_ptr(), x_out.data_ptr(), dead.data_ptr(), D, var, 5, 99, 40, B,
              R_rows, 1 if cplx else 0, _stream(dev))
    torch.cuda.synchronize(dev)
    got = out.read().double().reshape(B, C)  # (every owned word written, the guard words intact)
    assert not bool(torch.isnan(got).any())
    live = torch.isfinite(want).any(dim=1)
    has_rank1 = any(kd == S.KIND_RANK1 for _, _, _, _, sibs in levels for kd, _, _ in sibs)
    assert int((~live).sum()) == (1 if B > 1 and has_rank1 else 0) and bool(torch.isfinite(want[live]).all())
    assert float(S.log_share(want[live].numpy()).min()) >= S.MIN_LOG_SHARE  # (no state is left to a weaker criterion)
    _check(got, want, f"{shape} B={B}")  # (R.bound on the live states, -inf exactly on the all -inf row)
    # the draw: the restated inverse CDF, away from the boundaries
    u = S.uniform(S.philox4x32_10(np.arange(B, dtype=np.uint64) + np.uint64(40), 5, 0, 0, 99, 0)[0])
    state, cdf = S.draw(want.numpy().copy(), u)
    xo, xw = x_out.cpu(), x.cpu()
    others = [c for c in range(D) if c != var]
    assert bool((xo[:, others] == 7).all()) and bool((xw[:, others] == 7).all())
    for b in range(B):
        if state[b] < 0:
            assert int(xo[b, var]) == -1 and int(xw[b, var]) == 0 and int(dead[b]) == 1
            continue
        lo = cdf[b, state[b] - 1] if state[b] > 0 else -np.inf
        hi = cdf[b, state[b]] if state[b] < C - 1 else np.inf
        if min(u[b] - lo, hi - u[b]) > 4 * S.EPS:
            assert int(xo[b, var]) == state[b] and int(xw[b, var]) == state[b] and int(dead[b]) == 0
        else:
            assert 0 <= int(xo[b, var]) < C


# ---- 5. draw for draw -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "raster", "conditional"])
def test_draw_for_draw(hip_device, name):
    """2048 rows of the 32 signed units (16 steps) against the fp64 restated sampler: no differing row that is not near a
    boundary, differing share <= near share <= 2 %, observed entries exact, the same samples with another `rows_per_chunk`."""
    g = S.golden()
    sq = _emb32_circuit(str(hip_device))
    x, drawn, order, seed = S.draw_cases()[name]
    want, near = torch.from_numpy(g[f"draw_{name}_out"].astype(np.int64)), S.near_rows(g[f"draw_{name}_margin"])
    xd = x.to(hip_device)
    if name == "conditional":
        got = sq.sample_conditional(xd, torch.from_numpy(drawn), seed=seed)
        assert sq.last_mixed_launches > 0  # (scattered evidence)
        again = sq.sample_conditional(xd, np.nonzero(drawn)[0].tolist(), seed=seed, rows_per_chunk=700)
    else:
        got = sq.sample(S.DRAW_ROWS, seed=seed, order=order)
        assert (sq.last_mixed_launches > 0) == (name == "raster")
        again = sq.sample(S.DRAW_ROWS, seed=seed, order=order, rows_per_chunk=700)
    assert got.dtype == torch.int64 and got.shape == (S.DRAW_ROWS, 16) and torch.equal(got, again)
    got = got.cpu()
    assert bool((got[:, ~torch.from_numpy(drawn)] == x[:, ~torch.from_numpy(drawn)]).all())
    assert int(got.min()) >= 0 and int(got.max()) < 3
    differs = (got != want).any(dim=1).numpy()
    print(f"{name}: {int(differs.sum())} rows differ, {int(near.sum())} of {len(near)} are near a boundary")
    assert not bool((differs & ~near).any())
    assert differs.mean() <= near.mean() <= 0.02


# ---- 6. the exact distribution ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_samples_follow_the_enumerated_distribution(hip_device, sum_product):
    pytest.importorskip("scipy.stats")
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, states = R.tiny_case(sum_product)
    big, bt = R.pad_tiny_to_32(plan, tensors, sum_product)
    sq = HipSquaredCircuit(big, bt, device=hip_device)
    N = 1 << 18
    got = sq.sample(N, seed=20250105).cpu().numpy()
    assert got.min() >= 0 and sq.last_mixed_launches == 0
    p = torch.softmax(R.log_c2_of(plan, tensors, R.all_worlds(6, states)), dim=0).numpy()
    assert _chi2_p(np.bincount(S.world_codes(got, states), minlength=states ** 6), p * N) >= 1e-6


def test_conditional_samples_follow_the_enumerated_conditional(hip_device):
    pytest.importorskip("scipy.stats")
    plan, tensors, states = R.emb32_case()
    sq = _emb32_circuit(str(hip_device))
    N = 1 << 16
    q = [2, 7, 8, 13]
    row = R.rows_of(16, states, 1, seed=31)
    got = sq.sample_conditional(row.repeat(N, 1).to(hip_device), q, seed=20250106).cpu()
    rest = [v for v in range(16) if v not in q]
    assert bool((got[:, rest] == row[:, rest]).all())
    worlds = row.repeat(states ** 4, 1)
    worlds[:, q] = R.all_worlds(4, states)
    p = torch.softmax(R.log_c2_of(plan, tensors, worlds), dim=0).numpy()
    assert _chi2_p(np.bincount(S.world_codes(got[:, q].numpy(), states), minlength=states ** 4), p * N) >= 1e-6


# ---- 7. consistency past enumeration --------------------------------------------------------------------------------------
def test_chain_rule_on_the_8x8_image(hip_device):
    """64 pixels, 4 states, 32 units: the posteriors of the drawn states along the default order, 64 independently computed
    steps, sum to `log_prob`."""
    from cirkit_amd.squared import HipSquaredCircuit
    from cirkit_amd.squared_sampling import tree_order

    plan, tensors, states = R.img8_case()
    sq = HipSquaredCircuit(plan, tensors, device=hip_device)
    x = sq.sample(64, seed=20250107)
    assert int(x.min()) >= 0 and int(x.max()) < states
    order = tree_order(sq.plan)
    total = torch.zeros(64, dtype=torch.float64, device=hip_device)
    for i, v in enumerate(order):
        post = sq.posterior(x, v, order[i + 1:])
        total += post.gather(1, x[:, v: v + 1])[:, 0].double()
    want = sq.log_prob(x).cpu().double()
    err = (total.cpu() - want).abs()
    b = 64 * 2.0 * torch.from_numpy(R.bound(want))
    print(f"chain rule: worst error {float((err / b).max()):.3f} of the bound")
    assert bool((err <= b).all())


# ---- 8. refusals and edge rows ---------------------------------------------------------------------------------------------
def test_refusals_and_edge_rows(hip_device):
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.squared import HipSquaredCircuit
    from cirkit_amd.squared_sampling import path_plan
    from cirkit_amd.templates import InputSpec, build_plan, quad_graph

    plan, tensors, x = R.gauss_case()
    gs = HipSquaredCircuit(plan, tensors, device=hip_device)
    xg = x[:2].to(torch.float32).to(hip_device)
    for call in (lambda: gs.sample(4), lambda: gs.sample_conditional(xg, [1]), lambda: gs.state_log_marginals(xg, 1),
                 lambda: gs.posterior(xg, 1)):
        with pytest.raises(NotImplementedError, match="Gaussian"):
            call()
    assert bool(torch.isfinite(gs.log_marginal(xg, [5])).all())  # (what it offered before still works)
    dag = build_plan(quad_graph(4, 4), input_layer=InputSpec("embedding", 3), sum_product="cp", num_input_units=4, num_sum_units=4,
                     sum_activation="none", semiring="complex-lse-sum")
    with pytest.raises(NotImplementedError):  # (a QuadGraph mixes its partitions with sums of arity 2: refused as before, by the
        HipSquaredCircuit(dag, init_plan_tensors(dag, seed=3), device=hip_device)  # constructor; and its ancestries are no paths)
    with pytest.raises(NotImplementedError, match="DAG"):
        path_plan(dag, 5)
    sq = _emb32_circuit(str(hip_device))
    xd = torch.from_numpy(S.golden()["emb32_x"])[:4].to(hip_device)
    with pytest.raises(ValueError, match="permutation"):
        sq.sample(4, order=list(range(15)))
    with pytest.raises(ValueError, match="permutation"):
        sq.sample_conditional(xd, [1, 2], order=[1, 1])
    with pytest.raises(ValueError, match="permutation"):
        sq.sample_conditional(xd, [1, 2], order=[1, 3])
    with pytest.raises(ValueError, match="integrated out"):
        sq.state_log_marginals(xd, 3, [3, 4])
    ref = sq.state_log_marginals(xd, 5, [0, 1]).clone()
    bad = xd.clone()
    bad[1, 9] = -1  # observed
    bad[2, 0] = -7  # integrated: ignored
    bad[3, 5] = -2  # the variable itself: ignored
    got = sq.state_log_marginals(bad, 5, [0, 1])
    assert bool(torch.isnan(got[1]).all()) and torch.equal(got[[0, 2, 3]], ref[[0, 2, 3]])
    drawn = [0, 1, 5, 12]
    s_ref = sq.sample_conditional(xd, drawn, seed=5)
    s_bad = sq.sample_conditional(bad, drawn, seed=5)
    assert bool((s_bad[1, drawn] == -1).all()) and int(s_bad[1, 9]) == -1
    assert torch.equal(s_bad[[0, 2, 3]], s_ref[[0, 2, 3]])
    assert torch.equal(sq.sample_conditional(xd, drawn, seed=5), s_ref)  # a later valid call is unaffected
    assert torch.equal(sq.state_log_marginals(xd, 5, [0, 1]), ref)
