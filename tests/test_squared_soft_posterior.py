"""Posteriors and sampling under soft evidence of squared circuits on the GPU (cirkit_amd/squared_soft_posterior.py:
`HipSquaredCircuit.soft_query_log_marginals`, `soft_posterior_marginals`, `sample_soft`; the launches `ck_squared_soft_down_leaf`,
cirkit_amd/csrc/ck_sqsoftdown.hip, and `ck_squared_path_soft_bwd`, cirkit_amd/csrc/ck_sqpath.hip) against fp64 enumeration with the
repository's oracle: entry ``(b, v, s)`` is `RS.enumerated_soft` with the weights of ``v`` replaced by the indicator of ``s`` times
``lambda_v(s)`` (tests/squared_soft_posterior_restatement.py; its fp64 run is pinned to the enumeration and its fp32 run stays below
half the bound asserted here: tests/test_squared_soft_posterior_restatement.py, which also recomputes the recorded expectations in
tests/golden/sq_soft_posterior_expected.npz and asserts the share of states on the linear route).

Comparison (`P.check`): a state that holds at least e^-4 of its row's largest expected mass is held to
``|got - want| <= 1e-4 max(1, |want|)`` on the logarithm, the others to 4e-5 in linear space after the shift by the row's expected
maximum; the fp64 expectation decides which; a state whose expectation is -inf must be exactly -inf.  Between two GPU results
the bound is twice that.

Measured on an MI355X, worst error as a fraction of the bound: the tiny circuits 0.043, 32 signed units 0.060 (one soft pixel,
B = 3 and 33; worst linear error 2.5e-6), the plain leaf form on the same 0.059, the identities 0.054, the leaf kernel alone 0.004
(MFMA against plain 0.001); draw for draw 0 of 2048 rows differ (10 near a boundary), and with all-zero weights no row differs from
`sample_conditional` ("Posteriors and sampling under soft evidence of squared circuits")."""
import functools

import numpy as np
import pytest
import torch

import squared_down_restatement as P
import squared_marginal_restatement as R
import squared_sampling_restatement as S
import squared_soft_posterior_restatement as Q
import squared_soft_restatement as RS
from guarded_buffers import NEG_INF, _Guarded, _stream

pytestmark = pytest.mark.gpu


def _check(got, want, what="", factor=1.0):
    """`R.bound` on every finite value; the others exactly."""
    got = got.detach().cpu().double()
    want = torch.as_tensor(want).detach().cpu().double()
    fin = torch.isfinite(want)
    assert bool((got[~fin] == want[~fin]).all()), f"{what}: where the expected value is not finite"
    if not bool(fin.any()):
        return
    err = (got[fin] - want[fin]).abs()
    b = factor * torch.from_numpy(R.bound(want[fin]))
    print(f"{what}: worst error {float((err / b).max()):.3f} of the bound")
    assert bool((err <= b).all()), f"{what}: {float(err.max())} against {float(b.min())}"


def _identities(sq, ll, xd, s, m, route, what):
    """logsumexp over the states = the returned evidence = `soft_evidence_log_prob`, for every variable; posteriors sum to one."""
    got, ev = sq.soft_query_log_marginals(ll, xd, soft_vars=s, integrate_vars=m, normalized=False, return_log_evidence=True)
    z = sq.soft_evidence_log_prob(ll, xd, soft_vars=s, integrate_vars=m, normalized=False).cpu()
    _check(ev, z, f"{what}: the returned evidence", factor=2.0)
    _check(torch.logsumexp(got, dim=2), z[:, None].expand(-1, len(s)), f"{what}: summed over the states", factor=2.0)
    post, evn = sq.soft_posterior_marginals(ll, xd, soft_vars=s, integrate_vars=m, return_log_evidence=True)
    _check(torch.logsumexp(post, dim=2), torch.zeros(post.shape[:2]), f"{what}: posteriors sum to one", factor=2.0)
    _check(evn, sq.soft_evidence_log_prob(ll, xd, soft_vars=s, integrate_vars=m).cpu(), f"{what}: normalised evidence", factor=2.0)
    P.check(post, got.cpu() - torch.logsumexp(got.cpu().double(), dim=2, keepdim=True), f"{what}: posteriors", factor=2.0,
            route=route - torch.logsumexp(torch.as_tensor(route), dim=2, keepdim=True).numpy())
    return got


# ---- 1. the tiny circuits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [True, False], ids=["32units", "3units"])
@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_every_split_of_the_tiny_circuits(hip_device, sum_product, padded):
    """5 rows; K = 3 as it is (the plain leaf form) and padded to 32 units (the MFMA form: 3 states in a tile of 32)."""
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, x, cases = Q.tiny_expected(sum_product)
    if padded:
        plan, tensors = R.pad_tiny_to_32(plan, tensors, sum_product)
    sq = HipSquaredCircuit(plan, tensors, device=hip_device)
    xd = x.to(hip_device)
    for s, m, ll, want in cases:
        lld = ll.float().to(hip_device)
        got = sq.soft_query_log_marginals(lld, xd, soft_vars=s, integrate_vars=m, normalized=False)
        assert got.shape == (5, len(s), 3) and got.dtype == torch.float32 and sq.last_down_launches > 0 and sq.last_soft_launches > 0
        P.check(got, want, f"{sum_product} S={s} I={m}")
    s, m, ll, want = cases[-2]
    _identities(sq, ll.float().to(hip_device), xd, list(s), list(m), want.numpy(), f"{sum_product} S={s} I={m}")
    lz = float(sq.log_partition())
    P.check(sq.soft_query_log_marginals(ll.float().to(hip_device), xd, soft_vars=s, integrate_vars=m), want - lz, "normalised", factor=2.0)
    s, m, ll, want = cases[-1]  # S = all: x is not needed
    P.check(sq.soft_query_log_marginals(ll.float().to(hip_device), normalized=False), want, "S = all, no x")


# ---- 2. 32 signed units -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _emb32_circuit(dev, rows_per_block=1):
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, _ = R.emb32_case()
    return HipSquaredCircuit(plan, tensors, device=dev, rows_per_block=rows_per_block)


@pytest.mark.parametrize("B", [1, 3, 33])
def test_32_signed_units(hip_device, B):
    """One pixel, a 2 x 2 block, all 16, and {1, 6, 11, 12} with I = {3, 9}; the launch counters."""
    from cirkit_amd.squared_soft_posterior import plan_of

    g = Q.golden()
    sq = _emb32_circuit(str(hip_device))
    xd = Q.emb32_rows()[:B].to(hip_device)
    for i, (s, m) in enumerate(Q.EMB32_SPLITS):
        ll = Q.emb32_log_lik(i)[:B].float().to(hip_device)
        want = g[f"emb32_want_{i}"][:B]
        got = _identities(sq, ll, xd, list(s), list(m), want, f"B={B} S={s} I={m}")
        P.check(got, want, f"B={B} S={s} I={m}")
        got, ev = sq.soft_query_log_marginals(ll, xd, soft_vars=s, integrate_vars=m, return_log_evidence=True)
        dp = plan_of(sq, RS.mask_of(s, 16), RS.mask_of(m, 16))  # (the cached plan of this call)
        assert dp.qvars == sorted(s)
        assert sq.last_soft_launches == len(dp.mixed.leaves) == 1 and sq.last_launches == len(dp.mixed.layers)
        assert sq.last_down_launches == len(dp.layers) + 1


def test_the_plain_leaf_form_agrees_on_32_units(hip_device):
    from cirkit_amd.squared_soft_posterior import soft_query_log_marginals

    g = Q.golden()
    sq = _emb32_circuit(str(hip_device))
    xd = Q.emb32_rows().to(hip_device)
    for i, (s, m) in enumerate(Q.EMB32_SPLITS):
        ll = Q.emb32_log_lik(i).float().to(hip_device)
        a = soft_query_log_marginals(sq, ll, xd, soft_vars=s, integrate_vars=m, normalized=False, form=0)
        b = soft_query_log_marginals(sq, ll, xd, soft_vars=s, integrate_vars=m, normalized=False, form=1)
        P.check(b, g[f"emb32_want_{i}"], f"plain form S={s} I={m}")
        P.check(a, b, f"MFMA against plain S={s} I={m}", factor=2.0, route=g[f"emb32_want_{i}"])


def test_zero_weights_and_one_hot_weights(hip_device):
    """``log_lik = 0`` is `posterior_marginals(x, S, I)`; one-hot weights on S - v are `posterior(x', v, I)` with those observed."""
    sq = _emb32_circuit(str(hip_device))
    x = Q.emb32_rows()[:6]
    xd = x.to(hip_device)
    s, m = [1, 6, 11, 12], [3, 9]
    zero = torch.zeros(6, len(s), 3, device=hip_device)
    a, ev = sq.soft_query_log_marginals(zero, xd, soft_vars=s, integrate_vars=m, return_log_evidence=True)
    b, ev2 = sq.query_log_marginals(xd, s, m, return_log_evidence=True)
    want = P.expected_query_log_marginals(*R.emb32_case()[:2], x, s, m, 3).numpy() - float(sq.log_partition())
    P.check(a, b, "all-zero weights = query_log_marginals", factor=2.0, route=want)
    _check(ev, ev2.cpu(), "all-zero weights: the evidence", factor=2.0)
    P.check(sq.soft_posterior_marginals(zero, xd, soft_vars=s, integrate_vars=m), sq.posterior_marginals(xd, s, m), "all-zero = posterior_marginals",
            factor=2.0, route=want - torch.logsumexp(torch.from_numpy(want), dim=2, keepdim=True).numpy())
    for j, v in enumerate(s):
        hot = torch.full((6, len(s), 3), NEG_INF)
        hot.scatter_(2, x[:, s][:, :, None], 0.0)
        hot[:, j, :] = 0.0
        got = sq.soft_posterior_marginals(hot.to(hip_device), xd, soft_vars=s, integrate_vars=m)[:, j, :]
        one = sq.posterior(xd, v, m)
        mask = np.zeros(16, dtype=bool)
        mask[m] = True
        ref = S.enumerated_state_log_marginals(*R.emb32_case()[:2], x, v, mask, 3)
        P.check(got, one, f"one-hot on S - {v} = posterior", factor=2.0, route=(ref - torch.logsumexp(ref, dim=1, keepdim=True)).numpy())


# ---- 3. the Categorical fixture -------------------------------------------------------------------------------------------------
def test_real_circuit_under_lse_sum(hip_device):
    """`sq_cat_qt4x4_k5`: 256 states (two slabs of the MFMA form), K = 5 padded to 32, a table of logarithms, `float` values."""
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, _ = R.cat_case()
    sq = HipSquaredCircuit(plan, tensors, device=hip_device)
    assert sq.c._pad_info is not None and sq.plan.layers[1].num_input_units == 32
    s, m = Q.CAT_SPLIT
    got, ev = sq.soft_query_log_marginals(Q.cat_log_lik().float().to(hip_device), Q.cat_rows().to(hip_device), soft_vars=s, integrate_vars=m,
                                          normalized=False, return_log_evidence=True)
    assert got.shape == (3, 3, 256)
    # (no signed cancellation in this circuit: EVERY state is held to the bound on its logarithm, as tests/test_squared_posterior_marginals.py holds it)
    P.check(got, Q.golden()["cat_want"], f"S={s} I={m}", min_log_share=-np.inf)
    _check(torch.logsumexp(got, dim=2), ev.cpu()[:, None].expand(-1, 3), "summed over the states", factor=2.0)


# ---- 4. chunks and rows per workgroup ---------------------------------------------------------------------------------------------
def test_chunks_and_rows_per_block_do_not_change_a_bit(hip_device):
    sq = _emb32_circuit(str(hip_device))
    sq3 = _emb32_circuit(str(hip_device), 3)
    xd = Q.emb32_rows()[:5].to(hip_device)
    for i in (1, 3):
        s, m = Q.EMB32_SPLITS[i]
        ll = Q.emb32_log_lik(i)[:5].float().to(hip_device)
        ref, ev = (t.clone() for t in sq.soft_query_log_marginals(ll, xd, soft_vars=s, integrate_vars=m, return_log_evidence=True))
        for rpc in (1, 2):
            got, ev2 = sq.soft_query_log_marginals(ll, xd, soft_vars=s, integrate_vars=m, return_log_evidence=True, rows_per_chunk=rpc)
            assert torch.equal(got, ref) and torch.equal(ev2, ev)
        assert torch.equal(sq3.soft_query_log_marginals(ll, xd, soft_vars=s, integrate_vars=m), ref)
        assert torch.equal(sq.soft_posterior_marginals(ll, xd, soft_vars=s, integrate_vars=m, rows_per_chunk=2),
                           sq3.soft_posterior_marginals(ll, xd, soft_vars=s, integrate_vars=m))


# ---- 5. refusals and edge rows ----------------------------------------------------------------------------------------------------
def test_refusals_and_edge_rows(hip_device):
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, x = R.gauss_case()
    gs = HipSquaredCircuit(plan, tensors, device=hip_device)
    xg = x[:2].to(torch.float32).to(hip_device)
    w = torch.zeros(2, 1, 3, device=hip_device)
    for call in (lambda: gs.soft_query_log_marginals(w, xg, soft_vars=[1]), lambda: gs.soft_posterior_marginals(w, xg, soft_vars=[1]),
                 lambda: gs.sample_soft(w, xg, soft_vars=[1])):
        with pytest.raises(NotImplementedError, match="Gaussian"):
            call()
    assert not gs._soft_down_plans and getattr(gs, "_down_buf", None) is None  # (nothing was planned or allocated)
    sq = _emb32_circuit(str(hip_device))
    xd = Q.emb32_rows()[:4].to(hip_device)
    s, m = [0, 5, 6], [1]
    ll = (RS.log_lik_of(4, 3, 3, 77) * Q.WEIGHT_SCALE).float().to(hip_device)
    for call in (sq.soft_query_log_marginals, sq.soft_posterior_marginals, sq.sample_soft):
        with pytest.raises(ValueError, match="both soft and integrated"):
            call(ll, xd, soft_vars=[0, 5, 6], integrate_vars=[6])
        with pytest.raises(ValueError, match="at least one"):
            call(ll[:, :0], xd, soft_vars=[])
        with pytest.raises(ValueError, match="x is required"):
            call(ll, soft_vars=s, integrate_vars=m)
        with pytest.raises(ValueError):
            call(ll[:, :2], xd, soft_vars=s)  # (the S axis has 2 entries for 3 soft variables)
        with pytest.raises(ValueError, match="states"):
            call(ll[:, :, :2], xd, soft_vars=s)
        with pytest.raises(ValueError, match="rows"):
            call(ll, xd[:3], soft_vars=s)
    with pytest.raises(ValueError, match="permutation"):
        sq.sample_soft(ll, xd, soft_vars=s, order=[0, 5])
    with pytest.raises(NotImplementedError, match="drawn"):
        sq.sample_soft(torch.zeros(4, 16, 3, device=hip_device), order=list(range(16)))  # raster order: a sibling partly drawn
    ref, ev = (t.clone() for t in sq.soft_query_log_marginals(ll, xd, soft_vars=s, integrate_vars=m, return_log_evidence=True))
    s_ref = sq.sample_soft(ll, xd, soft_vars=s, integrate_vars=m, seed=5).clone()
    bad_x, bad_ll = xd.clone(), ll.clone()
    bad_ll[0, 1, :] = NEG_INF  # an all -inf variable: the row has no mass
    bad_ll[1, 2, 0] = float("nan")
    bad_x[2, 9] = -1  # observed
    bad_x[3, 5] = -2  # a soft variable: ignored
    bad_x[3, 1] = -7  # integrated: ignored
    got, ev2 = sq.soft_query_log_marginals(bad_ll, bad_x, soft_vars=s, integrate_vars=m, return_log_evidence=True)
    assert bool(torch.isneginf(got[0]).all()) and bool(torch.isneginf(ev2[0]))
    assert bool(torch.isnan(got[[1, 2]]).all()) and bool(torch.isnan(ev2[[1, 2]]).all())
    assert torch.equal(got[3], ref[3]) and torch.equal(ev2[3], ev[3])
    post = sq.soft_posterior_marginals(bad_ll, bad_x, soft_vars=s, integrate_vars=m)
    assert bool(torch.isnan(post[:3]).all()) and bool(torch.isfinite(post[3]).all())  # (a (row, variable) without mass is NaN)
    drawn = sq.sample_soft(bad_ll, bad_x, soft_vars=s, integrate_vars=m, seed=5)
    assert bool((drawn[:3][:, s] == -1).all()) and int(drawn[2, 9]) == -1 and torch.equal(drawn[3, s], s_ref[3, s])
    rest = [v for v in range(16) if v not in s]
    assert torch.equal(drawn[:, rest], bad_x[:, rest])  # observed entries untouched, integrated columns as given
    assert torch.equal(sq.soft_query_log_marginals(ll, xd, soft_vars=s, integrate_vars=m), ref)  # a later valid call is unaffected
    assert torch.equal(sq.sample_soft(ll, xd, soft_vars=s, integrate_vars=m, seed=5), s_ref)


# ---- 6. the leaf kernel alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 70, 131, 300])
@pytest.mark.parametrize("tlog", [False, True], ids=["linear", "log"])
@pytest.mark.parametrize("cplx", [False, True], ids=["float", "c32"])
def test_the_leaf_kernel_alone(hip_device, cplx, tlog, C):
    """`ck_squared_soft_down_leaf` between guard words against the fp64 quadratic form: both forms at K = 32, the plain form at
    K = 3 and 5; three variables of different C in one launch (the -inf tail columns), the last with offset -1; (B, rows per
    block) = (1, 1), (5, 3), (19, 20); the last row's G all -inf; weights with -inf.  C: below one tile, a ragged last tile, odd
    and two slabs, past `sp_leaf`'s 256-state chunk.  The MFMA form against the plain one within twice the bound."""
    from cirkit_amd import _capi as capi

    dev = hip_device
    Cs = Q.leaf_states(C)
    for K in Q.LEAF_UNITS:
        for B, rpb in Q.LEAF_ROWS:
            G, tables, ll, want = Q.leaf_case(cplx, tlog, K, C, B)
            nq, Cl, Cmax = len(Cs), ll.shape[2], ll.shape[2] + 1
            Gd = G.to(torch.complex64 if cplx else torch.float32).contiguous().to(dev)
            tds = [t.float().contiguous().to(dev) for t in tables]
            lld = ll.float().contiguous().to(dev)
            host = np.zeros((nq, 6), dtype=np.int64)
            for j in range(nq):
                host[j] = (tds[j].data_ptr(), Cs[j], K, 1 if tlog else 0, j * B * K * K if j < nq - 1 else -1, nq - 1 - j)
            lld = lld.flip(1).contiguous()  # (variable j reads position nq - 1 - j of the S axis)
            vd = torch.from_numpy(host).to(dev)
            results = {}
            for form in ((0, 1) if K == 32 else (1,)):
                out = _Guarded(B * nq * Cmax, dev)
                capi.call("ck_squared_soft_down_leaf", Gd.data_ptr(), Gd.numel(), host.ctypes.data, vd.data_ptr(), nq, Cmax, lld.data_ptr(), nq, Cl,
                          out.out.data_ptr(), B, rpb, 1 if cplx else 0, form, _stream(dev))
                torch.cuda.synchronize(dev)
                got = out.read().double().reshape(B, nq, Cmax)  # (every owned word written, the guard words intact)
                for j in range(nq):
                    assert bool(torch.isneginf(got[:, j, Cs[j]:]).all())
                if B > 1:
                    assert bool(torch.isneginf(got[B - 1, : nq - 1]).all())
                P.check(got, want, f"K={K} C={C} B={B} form={form}")
                results[form] = got
            if len(results) == 2:
                P.check(results[0], results[1], f"K={K} C={C} B={B}: MFMA against plain", factor=2.0, route=want)


@pytest.mark.parametrize("tlog", [False, True], ids=["linear", "log"])
@pytest.mark.parametrize("cplx", [False, True], ids=["float", "c32"])
def test_a_row_of_the_leaf_kernel_does_not_depend_on_its_place(hip_device, cplx, tlog):
    """The same 19 rows (131 states: two slabs, a ragged tile) with 1 and with 20 rows per block -- the MFMA form rounds them to 16
    and 32, so rows 16 .. 18 change their workgroup, their wave's turn and their slab's staging -- and the first 7 rows alone
    (another B): bit for bit the same, in both forms."""
    from cirkit_amd import _capi as capi

    dev = hip_device
    K, C, B = 32, 131, 19
    Cs = Q.leaf_states(C)
    G, tables, ll, _ = Q.leaf_case(cplx, tlog, K, C, B)
    nq, Cl, Cmax = len(Cs), ll.shape[2], ll.shape[2] + 1
    tds = [t.float().contiguous().to(dev) for t in tables]

    def run(rows, rpb, form):
        Gd = G[:, :rows].to(torch.complex64 if cplx else torch.float32).contiguous().to(dev)
        lld = ll[:rows].float().contiguous().to(dev)
        host = np.zeros((nq, 6), dtype=np.int64)
        for j in range(nq):
            host[j] = (tds[j].data_ptr(), Cs[j], K, 1 if tlog else 0, j * rows * K * K if j < nq - 1 else -1, j)
        vd = torch.from_numpy(host).to(dev)
        out = _Guarded(rows * nq * Cmax, dev)
        capi.call("ck_squared_soft_down_leaf", Gd.data_ptr(), Gd.numel(), host.ctypes.data, vd.data_ptr(), nq, Cmax, lld.data_ptr(), nq, Cl,
                  out.out.data_ptr(), rows, rpb, 1 if cplx else 0, form, _stream(dev))
        torch.cuda.synchronize(dev)
        return out.raw().reshape(rows, nq, Cmax)  # (the bits, guards checked)

    for form in (0, 1):
        ref = run(B, 1, form)
        assert torch.equal(run(B, 20, form), ref) and torch.equal(run(B, 3, form), ref)
        assert torch.equal(run(7, 1, form), ref[:7]) and torch.equal(run(7, 20, form), ref[:7])


def test_the_leaf_launch_checks_its_arguments(hip_device):
    from cirkit_amd import _capi as capi

    dev = hip_device
    t = torch.zeros(4, 32, device=dev)
    G = torch.zeros(2 * 1024, device=dev)
    ll = torch.zeros(2, 1, 3, device=dev)
    out = torch.zeros(2 * 3, device=dev)

    def call(row, S=1, Cl=3, down_elems=2048, form=0, rpb=1):
        host = np.asarray([row], dtype=np.int64)
        capi.call("ck_squared_soft_down_leaf", G.data_ptr(), down_elems, host.ctypes.data, torch.from_numpy(host).to(dev).data_ptr(), 1, 3,
                  ll.data_ptr(), S, Cl, out.data_ptr(), 2, rpb, 0, form, _stream(dev))

    good = (t.data_ptr(), 3, 32, 0, 0, 0)
    call(good)
    for kw, row in ((dict(), (t.data_ptr(), 3, 32, 0, 1, 0)), (dict(), (t.data_ptr(), 3, 32, 0, 0, 1)), (dict(Cl=2), good), (dict(form=2), good),
                    (dict(rpb=0), good), (dict(down_elems=2047), good), (dict(), (t.data_ptr(), 4, 32, 0, 0, 0)), (dict(), (0, 3, 32, 0, 0, 0))):
        with pytest.raises(ValueError):
            call(row, **kw)
    torch.cuda.synchronize(dev)


# ---- 7. sampling --------------------------------------------------------------------------------------------------------------------
def test_draw_for_draw(hip_device):
    """2048 rows of the 32 signed units, half the pixels soft, one integrated, the others observed, the default order, against the
    fp64 restated sampler: no differing row that is not near a boundary, differing share <= near share <= 2 %, observed entries
    exact, no draw outside the support, the same draws with another `rows_per_chunk`."""
    g = Q.golden()
    sq = _emb32_circuit(str(hip_device))
    x, soft, mask, ll, seed = Q.draw_case()
    want, near = torch.from_numpy(g["draw_out"].astype(np.int64)), S.near_rows(g["draw_margin"])
    xd, lld = x.to(hip_device), ll.float().to(hip_device)
    got = sq.sample_soft(lld, xd, soft_vars=torch.from_numpy(soft), integrate_vars=torch.from_numpy(mask), seed=seed)
    assert sq.last_soft_launches == 1 and sq.last_launches > 0
    again = sq.sample_soft(lld, xd, soft_vars=np.nonzero(soft)[0].tolist(), integrate_vars=np.nonzero(mask)[0].tolist(), seed=seed, rows_per_chunk=700)
    assert sq.last_soft_launches == 3
    assert got.dtype == torch.int64 and got.shape == (Q.DRAW_ROWS, 16) and torch.equal(got, again)
    got = got.cpu()
    assert bool((got[:, ~torch.from_numpy(soft)] == x[:, ~torch.from_numpy(soft)]).all())
    assert int(got[:, torch.from_numpy(soft)].min()) >= 0 and int(got.max()) < 3
    holes = torch.isneginf(ll).numpy()
    assert not holes[np.arange(Q.DRAW_ROWS)[:, None], np.arange(8)[None, :], got[:, torch.from_numpy(soft)].numpy()].any()
    differs = (got != want).any(dim=1).numpy()
    print(f"{int(differs.sum())} rows differ, {int(near.sum())} of {len(near)} are near a boundary")
    assert not bool((differs & ~near).any())
    assert differs.mean() <= near.mean() <= 0.02


def test_samples_follow_the_enumerated_joint(hip_device):
    """Four soft pixels, 2^16 rows of one evidence row, one exact -inf weight: chi-square against the enumerated
    ``p(x_S | lambda, x_O)``, and no draw outside the support."""
    from test_squared_sampling import _chi2_p

    pytest.importorskip("scipy.stats")
    sq = _emb32_circuit(str(hip_device))
    x, soft, ll, _ = Q.chi_case()
    p = Q.golden()["chi_joint"]
    q = list(Q.CHI_VARS)
    N = Q.CHI_ROWS
    got = sq.sample_soft(ll.float()[None].expand(N, -1, -1).to(hip_device), x[None].expand(N, -1).to(hip_device), soft_vars=q, seed=Q.CHI_SEED).cpu()
    rest = [v for v in range(16) if v not in q]
    assert bool((got[:, rest] == x[None, rest]).all()) and int(got.min()) >= 0
    assert not bool((got[:, q[1]] == 2).any())  # (the state of weight 0)
    assert _chi2_p(np.bincount(S.world_codes(got[:, q].numpy(), 3), minlength=81), p * N) >= 1e-6


def test_zero_weights_draw_what_sample_conditional_draws(hip_device):
    """``log_lik = 0``: the same draws as `sample_conditional` with the same seed and order, every row of the 2048.  The marginals
    of a step come from other launches here (the siblings still to draw are weighted Grams of weight 1, not constants of the
    partition-function circuit), so a draw whose u lies within fp32 rounding of a bin boundary could in principle differ; with
    this seed none does, and the kernels are deterministic."""
    sq = _emb32_circuit(str(hip_device))
    x, soft, _, _, seed = Q.draw_case()
    ids = np.nonzero(soft)[0].tolist()
    xd = x.to(hip_device)
    a = sq.sample_soft(torch.zeros(Q.DRAW_ROWS, len(ids), 3, device=hip_device), xd, soft_vars=ids, seed=seed)
    b = sq.sample_conditional(xd, ids, seed=seed)
    print(f"rows whose draws differ: {int((a != b).any(dim=1).sum())}")
    assert torch.equal(a, b)
