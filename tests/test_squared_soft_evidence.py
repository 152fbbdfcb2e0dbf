"""Soft and interval evidence of squared circuits on the GPU (cirkit_amd/squared_soft.py: `HipSquaredCircuit.soft_evidence_log_prob`,
`interval_log_prob`, `log_cdf`; the weighted Gram leaves: `ck_squared_soft_leaf`, cirkit_amd/csrc/ck_sqsoft.hip) against fp64
enumeration with the repository's oracle -- ``logsumexp(2 Re log c + sum_v log lambda)`` over every completion of the soft and the
integrated variables (tests/squared_soft_restatement.py, whose fp32 run stays below half the bound asserted here:
tests/test_squared_soft_restatement.py).

Bound: ``|got - want| <= 1e-4 max(1, |want|)`` on the log value, the project's bound for Z on the GPU; identities between two GPU
results use twice that.  Where the completions cannot be listed (all 16 pixels, five 256-state pixels) the expected value is the
fp64 restatement, pinned to the enumeration on the host."""
import functools

import numpy as np
import pytest
import torch

import squared_marginal_restatement as R
import squared_soft_restatement as RS
from guarded_buffers import NEG_INF, _Guarded, _stream

pytestmark = pytest.mark.gpu


def _check(got, want, what="", factor=1.0):
    got = got.detach().cpu().double()
    want = torch.as_tensor(want).double()
    err = (got - want).abs()
    b = factor * torch.from_numpy(R.bound(want))
    print(f"{what}: worst error {float((err / b).max()):.3f} of the bound")
    assert bool((err <= b).all()), f"{what}: {float(err.max())} against {float(b.min())}"


# ---- 1. the tiny circuits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [True, False], ids=["32units", "3units"])
@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_every_split_of_the_tiny_circuits(hip_device, sum_product, padded):
    """5 rows, random log weights, every subset S of three variables with M empty or one other variable; K = 3 as it is (the plain
    form) and padded to 32 (the MFMA form: 3 states leave the last step half empty)."""
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, x, cases = RS.tiny_expected(sum_product)
    log_z = R.enumerated_log_marginal(plan, tensors, x[:1], np.ones(6, dtype=bool), 3)[0]
    if padded:
        plan, tensors = R.pad_tiny_to_32(plan, tensors, sum_product)
    sq = HipSquaredCircuit(plan, tensors, device=hip_device)
    xd = x.to(hip_device)
    got = torch.stack([sq.soft_evidence_log_prob(ll.to(hip_device), xd, soft_vars=s, integrate_vars=m, normalized=False) for s, m, ll, _ in cases])
    _check(got, torch.stack([w for *_, w in cases]), "unnormalised")
    s, m, ll, want = cases[-1]
    _check(sq.soft_evidence_log_prob(ll.float(), xd, soft_vars=s, integrate_vars=m), want - log_z, "normalised")


# ---- 2. 32 signed units ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _emb32_circuit(dev, rows_per_block=1):
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors = RS.emb32_expected()[:2]
    return HipSquaredCircuit(plan, tensors, device=dev, rows_per_block=rows_per_block)


@pytest.mark.parametrize("B", [1, 3, 33])
def test_32_signed_units(hip_device, B):
    from cirkit_amd import _capi as capi
    from cirkit_amd.squared_soft import soft_plan

    plan, tensors, x, cases, log_z = RS.emb32_expected()
    sq = _emb32_circuit(str(hip_device))
    # the kinds that meet, in some product, a FULL child that comes from a leaf -- a soft input fold, here through the dense sum of
    # arity 1 that the `cp` layers put on every input fold -- on the tables the launches are built from
    meets = set()
    for s, m, _, _ in cases:
        mp = soft_plan(sq, RS.mask_of(m, 16), RS.mask_of(s, 16))
        from_leaf = {(lf.layer, j) for lf in mp.leaves for j in range(len(lf.folds))}  # (layer, position among its evaluated folds)
        assert from_leaf
        for la in mp.layers:
            for j in range(len(la.folds)):
                full = [h for h in range(la.kind.shape[1]) if la.kind[j, h] == capi.CK_SQ_FULL and tuple(la.src[j, h]) in from_leaf]
                if la.kind.shape[1] == 1 and full:
                    from_leaf.add((la.layer, j))
                meets |= {int(la.kind[j, g]) for h in full for g in range(la.kind.shape[1]) if g != h}
    assert meets == {capi.CK_SQ_RANK1, capi.CK_SQ_CONST, capi.CK_SQ_FULL}
    xd = x[:B].to(hip_device)
    for s, m, ll, want in cases:
        got = sq.soft_evidence_log_prob(ll[:B].to(hip_device), xd, soft_vars=s, integrate_vars=m, normalized=False)
        _check(got, want[:B], f"B={B} |S|={len(s)} M={list(m)}")
    s, m, ll, want = cases[3]  # all 16 pixels: x is not needed, soft_vars=None means all of them
    _check(sq.soft_evidence_log_prob(ll[:B].to(hip_device)), want[:B] - log_z, "normalised, S = all")


# ---- 3. the Categorical fixture -----------------------------------------------------------------------------------------------------
def test_real_circuit_under_lse_sum(hip_device):
    """`sq_cat_qt4x4_k5`: 256 states (two slabs), K = 5 padded to 32 by HipCircuit, a table of logarithms, `float` values."""
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, x, cases = RS.cat_expected()
    sq = HipSquaredCircuit(plan, tensors, device=hip_device)
    assert sq.c._pad_info is not None and sq.plan.layers[1].num_input_units == 32
    for s, m, ll, want in cases:
        got = sq.soft_evidence_log_prob(ll.to(hip_device), x.to(hip_device), soft_vars=s, integrate_vars=m, normalized=False)
        _check(got, want, f"S={list(s)} M={list(m)}")
    lo, hi = torch.full((3, 16), 100, dtype=torch.int64), torch.full((3, 16), 140, dtype=torch.int64)
    want = RS.enumerated_soft(plan, tensors, x, RS.interval_log_lik(lo, hi, (5,), 256), RS.mask_of((5,), 16), RS.mask_of((), 16), 256)
    _check(sq.interval_log_prob(lo.to(hip_device), hi.to(hip_device), x.to(hip_device), box_vars=[5], normalized=False), want, "pixel in 100..140")


# ---- 4. identities ---------------------------------------------------------------------------------------------------------------------
def test_identities(hip_device):
    plan, tensors, x, _, _ = RS.emb32_expected()
    sq = _emb32_circuit(str(hip_device))
    dev = hip_device
    xd = x[:6].to(dev)
    S, M = [1, 5, 6, 11], [2, 12]
    # one-hot weights are point evidence
    hot = torch.full((6, len(S), 3), NEG_INF)
    hot.scatter_(2, x[:6][:, S][:, :, None], 0.0)
    _check(sq.soft_evidence_log_prob(hot.to(dev), xd, soft_vars=S), sq.log_prob(xd).cpu(), "one-hot = log_prob", factor=2.0)
    _check(sq.soft_evidence_log_prob(hot.to(dev), xd, soft_vars=S, integrate_vars=M), sq.log_marginal(xd, M).cpu(), "one-hot = log_marginal", 2.0)
    # all-zero log weights integrate the variable out
    zero = torch.zeros(6, len(S), 3, device=dev)
    _check(sq.soft_evidence_log_prob(zero, xd, soft_vars=S, integrate_vars=M, normalized=False), sq.log_marginal(xd, S + M, normalized=False).cpu(),
           "all-zero = log_marginal", factor=2.0)
    # 0/1 weights are a box (some rows with -inf weights, one variable's interval a single state)
    g = torch.Generator().manual_seed(3)
    lo = torch.randint(0, 3, (6, 16), generator=g)
    hi = torch.maximum(lo, torch.randint(0, 3, (6, 16), generator=g))
    box = RS.interval_log_lik(lo, hi, S, 3).float()
    a = sq.soft_evidence_log_prob(box.to(dev), xd, soft_vars=S, integrate_vars=M, normalized=False)
    b = sq.interval_log_prob(lo.to(dev), hi.to(dev), xd, box_vars=S, integrate_vars=M, normalized=False)
    _check(a, b.cpu(), "0/1 weights = interval_log_prob", factor=2.0)
    _check(b, RS.enumerated_soft(plan, tensors, x[:6], box.double(), RS.mask_of(S, 16), RS.mask_of(M, 16), 3), "interval against enumeration")
    # a full-range box, normalised, is 0: explicit bounds and the sentinel
    full_lo, full_hi = torch.zeros(6, 16, dtype=torch.int64, device=dev), torch.full((6, 16), 2, dtype=torch.int64, device=dev)
    _check(sq.interval_log_prob(full_lo, full_hi), torch.zeros(6), "full box", factor=2.0)
    _check(sq.interval_log_prob(full_lo - 1, full_hi - 3), torch.zeros(6), "sentinel box", factor=2.0)
    # the masses of two disjoint intervals of one variable add up to their union's
    def box_of(v, l, h):
        blo, bhi = lo.clone(), hi.clone()
        blo[:, v], bhi[:, v] = l, h
        return sq.interval_log_prob(blo.to(dev), bhi.to(dev), xd, box_vars=S, integrate_vars=M, normalized=False)

    _check(torch.logaddexp(box_of(5, 0, 0), box_of(5, 1, 2)), box_of(5, 0, 2).cpu(), "disjoint intervals add up", factor=2.0)
    # the CDF does not decrease
    lower = x[:6].clone()
    upper = torch.minimum(lower + torch.randint(0, 2, lower.shape, generator=g), torch.tensor(2))
    c0, c1 = sq.log_cdf(lower.to(dev)).cpu().double(), sq.log_cdf(upper.to(dev)).cpu().double()
    assert bool((c1 >= c0 - 2e-4 * c0.abs().clamp(min=1.0)).all()) and bool((c1 <= 2e-4).all())
    _check(sq.log_cdf(torch.full((2, 16), 2, dtype=torch.int64, device=dev)), torch.zeros(2), "CDF at the top", factor=2.0)
    _check(sq.log_cdf(lower[:, :].to(dev), integrate_vars=M), sq.interval_log_prob(torch.zeros_like(lower).to(dev), lower.to(dev), integrate_vars=M).cpu(),
           "log_cdf = interval_log_prob(0, x)", factor=2.0)


# ---- 5. edge rows ------------------------------------------------------------------------------------------------------------------------
def test_edge_rows(hip_device):
    plan, tensors, x, cases, _ = RS.emb32_expected()
    sq = _emb32_circuit(str(hip_device))
    dev = hip_device
    s, m, ll, _ = cases[2]  # S = a 2 x 2 block, M = {15}
    xd = x[:6].to(dev)
    ref = sq.soft_evidence_log_prob(ll[:6].to(dev), xd, soft_vars=s, integrate_vars=m, normalized=False).cpu()
    bad = ll[:6].clone().float()
    bad[1, 2, :] = NEG_INF  # every state of one variable without weight: -inf, not NaN
    bad[2, 0, 1] = float("nan")
    bad[3, 3, 0] = float("inf")
    bad[4, 1, 2] = NEG_INF  # (one state without weight: an ordinary row)
    xb = xd.clone()
    xb[5, 7] = -1  # a negative entry at an observed variable
    xb[0, 4] = -5  # ... at a soft and at an integrated variable: ignored
    xb[0, 15] = -5
    got = sq.soft_evidence_log_prob(bad.to(dev), xb, soft_vars=s, integrate_vars=m, normalized=False).cpu()
    assert float(got[1]) == NEG_INF
    assert bool(torch.isnan(got[[2, 3, 5]]).all()) and not bool(torch.isnan(got[[0, 1, 4]]).any())
    assert torch.equal(got[0], ref[0]) and bool(torch.isfinite(got[4]))
    want4 = RS.enumerated_soft(plan, tensors, x[4:5], bad[4:5].double(), RS.mask_of(s, 16), RS.mask_of(m, 16), 3)
    _check(got[4:5], want4, "a state without weight")
    # entries past a variable's own count are never read: C = 5 > 3 with NaN behind the states
    wide = torch.full((6, 4, 5), float("nan"))
    wide[:, :, :3] = ll[:6].float()
    assert torch.equal(sq.soft_evidence_log_prob(wide.to(dev), xd, soft_vars=s, integrate_vars=m, normalized=False).cpu(), ref)
    # intervals: empty, clamped, the sentinel
    lo, hi = torch.zeros(6, 16, dtype=torch.int64), torch.full((6, 16), 2, dtype=torch.int64)
    lo[1, 4], hi[1, 4] = 2, 1  # empty
    lo[2, 4], hi[2, 4] = -7, 1  # clamped to 0 .. 1
    lo[3, 4], hi[3, 4] = 1, 99  # clamped to 1 .. 2
    lo[4, 4], hi[4, 4] = -1, -1  # the sentinel: the full range
    lo[5, 4], hi[5, 4] = 5, 9  # above every state: empty
    got = sq.interval_log_prob(lo.to(dev), hi.to(dev), xd, box_vars=s, integrate_vars=m, normalized=False).cpu()
    assert float(got[1]) == NEG_INF and float(got[5]) == NEG_INF
    clo, chi = lo.clone(), hi.clone()
    clo[2, 4], chi[3, 4], clo[4, 4], chi[4, 4] = 0, 2, 0, 2
    rows = [0, 2, 3, 4]
    want = RS.enumerated_soft(plan, tensors, x[rows], RS.interval_log_lik(clo[rows], chi[rows], s, 3), RS.mask_of(s, 16), RS.mask_of(m, 16), 3)
    _check(got[rows], want, "clamped bounds and the sentinel")
    with pytest.raises(NotImplementedError, match="Gaussian layer"):  # (before anything is allocated)
        from cirkit_amd.squared import HipSquaredCircuit

        gplan, gtensors, gx = R.gauss_case()
        gsq = HipSquaredCircuit(gplan, gtensors, device=dev)
        gsq.soft_evidence_log_prob(torch.zeros(3, 1, 4, device=dev), gx[:3].float().to(dev), soft_vars=[5])


# ---- 6. the kernel alone -------------------------------------------------------------------------------------------------------------------
def _gram_case(K, C, B, n, tlog, seed, signed):
    g = torch.Generator().manual_seed(seed)
    F = n + 2
    if tlog:
        table = torch.randn(F, C + 1, K, generator=g, dtype=torch.float64) - 3
        table[0, :, K - 1] = NEG_INF  # a unit without mass: its row and column are -inf
    else:
        table = torch.randn(F, C + 1, K, generator=g, dtype=torch.float64)
        if not signed:  # (`float` values have no logarithm of a negative sum: a linear table under lse-sum is positive)
            table = table.abs()
    table[:, C, :] = float("nan")  # the integral row is not read
    folds = torch.randperm(F, generator=g)[:n].tolist()
    S = n + 1
    cols = torch.randperm(S, generator=g)[:n].tolist()
    ll = torch.rand(B, S, C + 2, generator=g, dtype=torch.float64) * 8 - 4
    ll[:, :, C:] = float("nan")  # entries past the states are not read
    ll[0, cols[0], :] = NEG_INF  # a row without any weight
    ll[B - 1, cols[0], : C // 2] = NEG_INF
    return table, folds, cols, ll


def _gram_reference(table, folds, cols, w, tlog, C):
    """(n, B, K, K) fp64 Gram in linear space relative to the shifts the kernel uses, the shifts (n, B, K, K), and the sum of
    the absolute terms: w (B, columns, C) linear weights already shifted by their row maximum m (B, columns)."""
    big = torch.finfo(torch.float32).max
    G, A, sh = [], [], []
    for f, c in zip(folds, cols):
        t = table[f, :C]
        if tlog:
            mt = t.amax(dim=0).clamp(min=-big, max=big)
            a = torch.exp(t - mt)
            s = mt[:, None] + mt[None, :]
        else:
            a, s = t, torch.zeros(t.shape[1], t.shape[1], dtype=torch.float64)
        G.append(torch.einsum("bs,sk,sl->bkl", w[:, c], a, a))
        A.append(torch.einsum("bs,sk,sl->bkl", w[:, c], a.abs(), a.abs()))
        sh.append(s)
    return torch.stack(G), torch.stack(A), torch.stack(sh)


@pytest.mark.parametrize("interval", [False, True], ids=["soft", "box"])
@pytest.mark.parametrize("K,C,B,n,R_rows,form", [(32, 3, 5, 1, 1, 0), (32, 131, 19, 2, 3, 0), (32, 70, 19, 2, 20, 0), (32, 70, 5, 2, 1, 1),
                                                 (5, 300, 5, 2, 3, 0), (3, 3, 4, 1, 1, 0)])
@pytest.mark.parametrize("tlog", [False, True], ids=["linear", "log"])
@pytest.mark.parametrize("cplx", [False, True], ids=["float", "c32"])
def test_kernel_alone(hip_device, cplx, tlog, K, C, B, n, R_rows, form, interval):
    """`ck_squared_soft_leaf` between guard words: the MFMA form (odd state counts, two slabs, one slab walked by two tiles of one
    workgroup, B no multiple of the rows of a workgroup, n = 1) and the plain form (K = 5 over two slabs, K = 3, and K = 32 forced),
    both element types, linear tables and tables of logarithms, soft weights and bounds.  Every Gram element against its fp64
    value in LINEAR space: fp32 accumulation of C terms is off by at most (C + 8) 2^-24 of the sum of their absolute values; the
    logarithm, the sums of the shifts and the final sum are up to six roundings of values below 16 in magnitude (an ulp there is
    9.5e-7: 6e-6 relative in linear space), the exponentials of the weights and of the table another 1e-6 at most: 8e-6."""
    from cirkit_amd import _capi as capi

    dev = hip_device
    table, folds, cols, ll = _gram_case(K, C, B, n, tlog, 17 * K + C + B, cplx)
    big = torch.finfo(torch.float32).max
    D = ll.shape[1]
    if interval:
        g = torch.Generator().manual_seed(C)
        lo = torch.randint(0, C, (B, D), generator=g)
        hi = torch.minimum(lo + torch.randint(0, C, (B, D), generator=g), torch.tensor(C + 3))
        lo[0, cols[0]], hi[0, cols[0]] = 2, 1  # empty
        lo[1 % B, cols[0]], hi[1 % B, cols[0]] = -1, -1  # the full range
        lo[2 % B, cols[0]] = -4
        l2 = torch.where((lo < 0) & (hi < 0), 0, lo.clamp(min=0))
        h2 = torch.where((lo < 0) & (hi < 0), C - 1, hi.clamp(max=C - 1))
        s = torch.arange(C)[None, None, :]
        w = ((s >= l2[:, :, None]) & (s <= h2[:, :, None])).double()
        m = torch.zeros(B, D, dtype=torch.float64)
    else:
        l32 = ll.float().double()
        m = l32[:, :, :C].amax(dim=2).clamp(min=-big, max=big)
        w = torch.exp(l32[:, :, :C] - m[:, :, None])
    t32 = table.float()
    G, A, sh = _gram_reference(t32.double(), folds, cols, w, tlog, C)
    e = 2 if cplx else 1
    out = _Guarded(n * B * K * K * e, dev)
    tab = np.ascontiguousarray(np.stack([folds, cols], axis=1).astype(np.int32))
    tab_d = torch.from_numpy(tab).to(dev)
    t_d = t32.contiguous().to(dev)
    mt_d = t32[:, :C].amax(dim=1).clamp(min=-big, max=big).contiguous().to(dev) if tlog else None
    ll_d = None if interval else ll.float().contiguous().to(dev)
    lo_d, hi_d = (lo.contiguous().to(dev), hi.contiguous().to(dev)) if interval else (None, None)
    capi.call("ck_squared_soft_leaf", t_d.data_ptr(), int(t_d.shape[0]), C, K, 1 if tlog else 0, None if mt_d is None else mt_d.data_ptr(),
              tab.ctypes.data, tab_d.data_ptr(), n, None if interval else ll_d.data_ptr(), 0 if interval else D, 0 if interval else C + 2,
              lo_d.data_ptr() if interval else None, hi_d.data_ptr() if interval else None, D if interval else 0, out.out.data_ptr(), B,
              R_rows, 1 if cplx else 0, form, _stream(dev))
    torch.cuda.synchronize(dev)
    got = out.read().double().reshape(n, B, K, K, e)
    shift = sh[:, None] + torch.stack([m[:, c] for c in cols])[:, :, None, None]
    lin = torch.exp(got[..., 0] - shift)  # |G| relative to the shifts
    dead = shift < -1e30  # (a unit without mass, a row without weight: shifted by -FLT_MAX, the value is -inf)
    assert bool((got[..., 0][dead] == NEG_INF).all()) and not bool(torch.isnan(got).any())
    if cplx:
        neg = (torch.remainder(got[..., 1], 2 * np.pi) - np.pi).abs() < 1e-3
        assert bool((neg | (got[..., 1].abs() < 1e-3)).all())
        lin = torch.where(neg, -lin, lin)
    tol = ((C + 8) * 2.0 ** -24 + 8e-6) * A
    err = (lin - G).abs()
    assert bool((err[~dead] <= tol[~dead] + 1e-300).all()), float((err[~dead] / (tol[~dead] + 1e-300)).max())
    assert bool((got[:, 0, :, :, 0][[0]] == NEG_INF).all())  # row 0 of fold 0: no weight / an empty interval


def test_kernel_refuses_what_does_not_fit(hip_device):
    from cirkit_amd import _capi as capi

    t = torch.zeros(1, 3, 65, device=hip_device)
    tab = np.zeros((1, 2), dtype=np.int32)
    ll = torch.zeros(1, 1, 2, device=hip_device)
    out = torch.empty(65 * 65, device=hip_device)
    args = lambda tb: ("ck_squared_soft_leaf", t.data_ptr(), 1, 2, 65, 0, None, tb.ctypes.data, torch.from_numpy(tb).to(hip_device).data_ptr(), 1,  # noqa: E731
                       ll.data_ptr(), 1, 2, None, None, 0, out.data_ptr(), 1, 1, 0, 0, _stream(hip_device))
    with pytest.raises(NotImplementedError, match="K=65"):
        capi.call(*args(tab))
    with pytest.raises(ValueError, match="table fold 1 of 1"):
        capi.call(*args(np.asarray([[1, 0]], dtype=np.int32)))


# ---- 7. chunking and launch counts ------------------------------------------------------------------------------------------------------
def test_chunking_and_launch_counts(hip_device):
    from cirkit_amd.squared_soft import soft_plan

    plan, tensors, x, cases, _ = RS.emb32_expected()
    sq = _emb32_circuit(str(hip_device))
    sq3 = _emb32_circuit(str(hip_device), 3)  # (rows walked per workgroup: the same bits)
    xd = x[:5].to(hip_device)
    lo = torch.zeros(5, 16, dtype=torch.int64, device=hip_device)
    for s, m, ll, _ in (cases[0], cases[2]):
        lld = ll[:5].to(hip_device)
        ref = sq.soft_evidence_log_prob(lld, xd, soft_vars=s, integrate_vars=m).clone()
        mp = soft_plan(sq, RS.mask_of(m, 16), RS.mask_of(s, 16))
        assert sq.last_soft_launches == len(mp.leaves) == 1 and sq.last_launches == len(mp.layers) > 0
        box = sq.interval_log_prob(lo, lo + 1, xd, box_vars=s, integrate_vars=m).clone()
        assert sq.last_soft_launches == 1 and sq.last_launches == len(mp.layers)
        for rpc in (1, 2):
            assert torch.equal(sq.soft_evidence_log_prob(lld, xd, soft_vars=s, integrate_vars=m, rows_per_chunk=rpc), ref)
            assert sq.last_soft_launches == -(-5 // rpc) and sq.last_launches == -(-5 // rpc) * len(mp.layers)
            assert torch.equal(sq.interval_log_prob(lo, lo + 1, xd, box_vars=s, integrate_vars=m, rows_per_chunk=rpc), box)
        assert torch.equal(sq3.soft_evidence_log_prob(lld, xd, soft_vars=s, integrate_vars=m), ref)
        assert torch.equal(sq3.interval_log_prob(lo, lo + 1, xd, box_vars=s, integrate_vars=m), box)
