"""Exact marginals and conditionals of squared circuits on the GPU (cirkit_amd/squared.py: `HipSquaredCircuit`; the mixed
folds: `ck_squared_mixed_fwd`, cirkit_amd/csrc/ck_sqmar.hip) against fp64 enumeration with the repository's oracle --
``logsumexp(2 Re log c)`` over every completion of the missing variables (tests/squared_marginal_restatement.py, whose fp32
run stays below a quarter of the bound asserted here: tests/test_squared_marginal_restatement.py).

Bound: ``|got - want| <= 1e-4 max(1, |want|)`` on the log value, the project's bound for Z on the GPU
(tests/test_functional.py); identities between two GPU results use twice that.  Where the completions cannot be enumerated
the expected value is: Z from the oracle's fp64 run of the partition-function plan (everything missing: 3^16 worlds), the fp64
restatement (three or more 256-state pixels of the Categorical fixture; pinned to the enumeration on the host), fp64 trapezoid
quadrature (Gaussian)."""
import functools

import numpy as np
import pytest
import torch

import squared_marginal_restatement as R
from guarded_buffers import NAN_BITS, NEG_INF, _GuardedArena, _stream

pytestmark = pytest.mark.gpu


def _masks6():
    return [np.array([(i >> v) & 1 for v in range(6)], dtype=bool) for i in range(64)]


def _check(got, want, what="", factor=1.0):
    got = got.detach().cpu().double()
    want = torch.as_tensor(want).double()
    err = (got - want).abs()
    b = factor * torch.from_numpy(R.bound(want))
    print(f"{what}: worst error {float((err / b).max()):.3f} of the bound")
    assert bool((err <= b).all()), f"{what}: {float(err.max())} against {float(b.min())}"


@functools.lru_cache(maxsize=None)
def _tiny_expected(sum_product):
    plan, tensors, states = R.tiny_case(sum_product)
    x = R.rows_of(6, states, 5)
    log_z = R.enumerated_log_marginal(plan, tensors, x[:1], np.ones(6, dtype=bool), states)[0]
    return plan, tensors, x, log_z, [R.enumerated_log_marginal(plan, tensors, x, m, states) for m in _masks6()]


@pytest.mark.parametrize("padded", [True, False], ids=["32units", "3units"])
@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_every_mask_of_the_tiny_circuits(hip_device, sum_product, padded):
    """All 64 masks, 5 rows; K = 3 padded to 32 units (the specialised forms) and as it is (the shape-generic form)."""
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, x, log_z, want = _tiny_expected(sum_product)
    if padded:
        plan, tensors = R.pad_tiny_to_32(plan, tensors, sum_product)
    sq = HipSquaredCircuit(plan, tensors, device=hip_device)
    xd = x.to(hip_device)
    _check(sq.log_partition().reshape(1), log_z.reshape(1), "log Z")
    got = torch.stack([sq.log_marginal(xd, torch.from_numpy(m), normalized=False) for m in _masks6()])
    _check(got, torch.stack(want), "unnormalised")
    got = torch.stack([sq.log_marginal(xd, torch.from_numpy(m)) for m in _masks6()[::7]])
    _check(got, torch.stack(want[::7]) - log_z, "normalised")
    _check(sq.log_prob(xd), want[0] - log_z, "log_prob")


@functools.lru_cache(maxsize=None)
def _emb32():
    plan, tensors, states = R.emb32_case()
    x = R.rows_of(16, states, 33)
    masks = R.masks_4x4()
    return plan, tensors, x, masks, [R.enumerated_log_marginal(plan, tensors, x, m, states) for m in masks], R.oracle_log_z(plan, tensors)


@functools.lru_cache(maxsize=None)
def _emb32_circuit(dev):
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors = _emb32()[:2]
    return HipSquaredCircuit(plan, tensors, device=dev)


@pytest.mark.parametrize("B", [1, 3, 33])
def test_32_signed_units(hip_device, B):
    from cirkit_amd import _capi as capi

    plan, tensors, x, masks, want, log_z = _emb32()
    sq = _emb32_circuit(str(hip_device))
    pairs = set()
    for m in masks:  # every pair of child kinds meets in some Hadamard product, on the tables the launches read
        for la in sq.classify(torch.from_numpy(m)).layers:
            for row in la.kind.tolist():
                pairs |= {tuple(sorted((a, b))) for i, a in enumerate(row) for b in row[i + 1:]}
    f, c, r = capi.CK_SQ_FULL, capi.CK_SQ_CONST, capi.CK_SQ_RANK1
    assert pairs == {tuple(sorted(p)) for p in ((r, c), (r, f), (c, f), (f, f))}
    xd = x[:B].to(hip_device)
    for m, w in zip(masks, want):
        _check(sq.log_marginal(xd, np.nonzero(m)[0].tolist(), normalized=False), w[:B], f"B={B} M={np.nonzero(m)[0].tolist()}")
    _check(sq.log_marginal(xd, torch.from_numpy(masks[4])), want[4][:B] - log_z, "normalised")
    assert sq.log_marginal(xd, []).shape == (B,) and sq.last_launches == 0  # nothing missing: c's forward alone
    sq.log_marginal(xd, range(16))
    assert sq.last_launches == 0  # everything missing: the constant root
    sq.log_marginal(xd, [0])
    assert sq.last_launches == 4  # the ancestors of pixel 0 over more than one pixel: one fold in each of the four CP-T layers


def test_chunking_does_not_change_a_bit(hip_device):
    plan, tensors, x, masks, _, _ = _emb32()
    sq = _emb32_circuit(str(hip_device))
    xd = x[:5].to(hip_device)
    for m in (masks[4], masks[2]):
        ref = sq.log_marginal(xd, torch.from_numpy(m)).clone()
        for rpc in (1, 2):
            assert torch.equal(sq.log_marginal(xd, torch.from_numpy(m), rows_per_chunk=rpc), ref)
    sq2 = type(sq)(plan, tensors, device=hip_device, rows_per_block=3)  # (rows walked per workgroup: the same bits too)
    assert torch.equal(sq2.log_marginal(xd, torch.from_numpy(masks[4])), sq.log_marginal(xd, torch.from_numpy(masks[4])))


def test_real_circuit_under_lse_sum(hip_device):
    """The `sq_cat_qt4x4_k5` fixture, K = 5 padded to 32 by HipCircuit: the `float` kernels."""
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, states = R.cat_case()
    x = torch.from_numpy(np.random.default_rng(2).integers(0, states, size=(3, 16)))
    sq = HipSquaredCircuit(plan, tensors, device=hip_device)
    assert sq.c._pad_info is not None and sq.plan.layers[1].num_input_units == 32
    log_z = R.oracle_log_z(plan, tensors)
    _check(sq.log_partition().reshape(1), log_z.reshape(1), "log Z")
    for m in R.masks_4x4(most=5):
        want = R.yardstick(plan, tensors, x, m, states)
        _check(sq.log_marginal(x.to(hip_device), torch.from_numpy(m), normalized=False), want, f"M={np.nonzero(m)[0].tolist()}")
    _check(sq.log_prob(x.to(hip_device)), R.log_c2_of(plan, tensors, x) - log_z, "log_prob")


def test_gaussian_inputs(hip_device):
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, x = R.gauss_case()
    x = x[:3]
    sq = HipSquaredCircuit(plan, tensors, device=hip_device)
    xd = x.to(torch.float32).to(hip_device)
    log_z = R.oracle_log_z(plan, tensors)
    _check(sq.log_marginal(xd, range(16)), torch.zeros(3), "all missing")
    _check(sq.log_marginal(xd, []), R.log_c2_of_float(plan, tensors, x) - log_z, "none missing")
    want, moved = R.gauss_quadrature(plan, tensors, x, 5)
    assert float(moved) < 1e-9  # the grid is accepted only if doubling it moves the integral by less than that
    _check(sq.log_marginal(xd, [5], normalized=False), want, "one missing against quadrature")


def test_marginal_consistency_past_enumeration(hip_device):
    """8 x 8 pixels, 4 states, 32 units: summing a marginal over the states of one more variable is the marginal without
    it; a conditional is the difference of two marginals and sums to one over its query variables."""
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, states = R.img8_case()
    sq = HipSquaredCircuit(plan, tensors, device=hip_device)
    x = R.rows_of(64, states, 4).to(hip_device)
    for mask, extra in R.img8_masks():
        mt = torch.from_numpy(mask)
        for v in extra:
            terms = []
            for s in range(states):
                xs = x.clone()
                xs[:, v] = s
                terms.append(sq.log_marginal(xs, mt, normalized=False))
            more = mask.copy()
            more[v] = True
            _check(torch.logsumexp(torch.stack(terms), dim=0), sq.log_marginal(x, torch.from_numpy(more), normalized=False).cpu(),
                   f"sum over variable {v}", factor=2.0)
        q = extra[:2]
        qm = mask.copy()
        qm[q] = True
        cond = sq.conditional_log_prob(x, q, mt)
        _check(cond, (sq.log_marginal(x, mt, normalized=False) - sq.log_marginal(x, torch.from_numpy(qm), normalized=False)).cpu(),
               "conditional", factor=2.0)
        total = []
        for s0 in range(states):
            for s1 in range(states):
                xs = x.clone()
                xs[:, q[0]], xs[:, q[1]] = s0, s1
                total.append(sq.conditional_log_prob(xs, q, mt))
        _check(torch.logsumexp(torch.stack(total), dim=0), torch.zeros(4), "conditional sums to one", factor=2.0)


def test_refusals_and_edge_rows(hip_device):
    from cirkit_amd.squared import HipSquaredCircuit
    from cirkit_amd.templates import image_data

    plan, tensors, x, masks, want, _ = _emb32()
    sq = _emb32_circuit(str(hip_device))
    xd = x[:4].to(hip_device)
    with pytest.raises(ValueError, match="ONE scope"):
        sq.log_marginal(xd, torch.zeros((4, 16), dtype=torch.bool))
    with pytest.raises(ValueError, match="subset of the circuit scope"):
        sq.log_marginal(xd, [3, 16])
    with pytest.raises(ValueError, match="torch.bool"):
        sq.log_marginal(xd, torch.zeros(16))
    with pytest.raises(ValueError, match="16 variables"):
        sq.log_marginal(xd, torch.zeros(15, dtype=torch.bool))
    with pytest.raises(ValueError):
        sq.conditional_log_prob(xd, [1], [1, 2])
    name = next(iter(plan.tensors))
    with pytest.raises(NotImplementedError, match="complex parameter"):
        HipSquaredCircuit(plan, {**tensors, name: np.asarray(tensors[name]).astype(np.complex64)}, device=hip_device)
    tucker = image_data((1, 4, 4), "quad-tree-2", num_input_units=2, sum_product_layer="tucker", num_sum_units=2)
    from cirkit_amd.initializers import init_plan_tensors

    with pytest.raises(NotImplementedError, match="tucker"):
        HipSquaredCircuit(tucker, init_plan_tensors(tucker, seed=1), device=hip_device)
    m = masks[4]  # a negative entry at an observed variable: that row alone is NaN; at a missing variable it is ignored
    bad = xd.clone()
    obs, mis = int(np.nonzero(~m)[0][0]), int(np.nonzero(m)[0][0])
    bad[1, obs] = -1
    bad[2, mis] = -7
    got = sq.log_marginal(bad, torch.from_numpy(m), normalized=False).cpu()
    assert bool(torch.isnan(got[1])) and not bool(torch.isnan(got[[0, 2, 3]]).any())
    ref = sq.log_marginal(xd, torch.from_numpy(m), normalized=False).cpu()
    assert torch.equal(got[[0, 2, 3]], ref[[0, 2, 3]])


def test_config_5_lower_half_missing(hip_device):
    """BASELINE config 5 (784 pixels, K = 32): finite with the lower half missing, `log_prob` with nothing missing, 0 with
    everything missing."""
    from conftest import load_case
    from cirkit_amd.squared import HipSquaredCircuit

    plan, tensors, g = load_case("cfg5_sos_c_k32")
    sq = HipSquaredCircuit(plan, tensors, device=hip_device)
    x = torch.from_numpy(g["x"].astype(np.int64))[:4].to(hip_device)
    lower = torch.zeros(784, dtype=torch.bool)
    lower[392:] = True
    got = sq.log_marginal(x, lower)
    assert bool(torch.isfinite(got).all()) and sq.last_launches > 0
    lp = sq.log_prob(x).cpu()
    _check(sq.log_marginal(x, []), lp, "empty mask", factor=2.0)
    assert bool((got.cpu() >= lp - 1e-3).all())  # a marginal is at least the probability of any completion
    _check(sq.log_marginal(x, torch.ones(784, dtype=torch.bool)), torch.zeros(4), "full mask", factor=2.0)


# ---- the kernel alone --------------------------------------------------------------------------------------------------------
def _stage_ref(v, w):
    return R._stage(v, w)


@pytest.mark.parametrize("B,R_rows", [(1, 1), (3, 2)])
@pytest.mark.parametrize("shape", ["all32", "root", "generic", "hadamard"])
@pytest.mark.parametrize("cplx", [False, True], ids=["float", "c32"])
def test_kernel_alone(hip_device, cplx, shape, B, R_rows):
    """`ck_squared_mixed_fwd` on a hand-built list of two folds with H = 2: fold 0 = (full, const), fold 1 = (rank-1, full);
    row 0 of the rank-1 child is all -inf (the clamped maximum: the result is -inf, not NaN).  The output lies between guard
    words inside the arena the full children live in: every owned word is written, no other word changes."""
    from cirkit_amd import _capi as capi

    dev = hip_device
    g = torch.Generator().manual_seed(5 + B)
    Ki = 3 if shape == "generic" else 32
    Ko = {"all32": 32, "root": 1, "generic": 2, "hadamard": Ki}[shape]
    stages = 0 if shape == "hadamard" else 2
    e = 2 if cplx else 1  # words per value
    K2, O2 = Ki * Ki, (Ki * Ki if stages == 0 else Ko * Ko)

    def values(*sh):
        re = torch.randn(*sh, generator=g, dtype=torch.float64)
        if not cplx:
            return re
        return torch.complex(re, torch.where(torch.rand(*sh, generator=g) < 0.5, 0.0, np.pi).double() + 0.1 * torch.randn(*sh, generator=g, dtype=torch.float64))

    fullA, fullB, cst, rk = values(B, K2), values(B, K2), values(K2), values(B, Ki)
    rk[0] = complex(NEG_INF, 0.0) if cplx else NEG_INF
    w = torch.randn(3, max(Ko, 1), Ki, generator=g, dtype=torch.float64)
    if not cplx:
        w = w.abs() + 0.05
    wfold = [2, 0]

    def words(t):
        t = t.to(torch.complex64 if cplx else torch.float32).contiguous()
        return (torch.view_as_real(t) if cplx else t).reshape(-1).float()

    n = 2
    out_words = n * B * O2 * e
    arena = _GuardedArena([B * K2 * e, B * K2 * e, out_words], dev, lead=0)
    arena.fill([words(fullA), words(fullB), torch.full((out_words,), NAN_BITS, dtype=torch.int32).view(torch.float32)])
    cst_d, rk_d, w_d = words(cst).to(dev), words(rk).to(dev), w.float().contiguous().to(dev)
    kind = torch.tensor([[capi.CK_SQ_FULL, capi.CK_SQ_CONST], [capi.CK_SQ_RANK1, capi.CK_SQ_FULL]], dtype=torch.int32, device=dev)
    off = torch.tensor([[arena.off[0] // e, 0], [0, arena.off[1] // e]], dtype=torch.int64, device=dev)
    wf = torch.tensor(wfold, dtype=torch.int32, device=dev)
    mid = torch.empty(max(1, n * B * Ki * Ko * e), dtype=torch.float32, device=dev)
    capi.call("ck_squared_mixed_fwd", arena.ptr(), cst_d.data_ptr(), rk_d.data_ptr(), kind.data_ptr(), off.data_ptr(), 2,
              w_d.data_ptr(), w_d.data_ptr(), wf.data_ptr(), mid.data_ptr(), arena.ptr() + 4 * arena.off[2], n, B, Ki, Ko, stages,
              R_rows, 1 if cplx else 0, _stream(dev))
    torch.cuda.synchronize(dev)
    host = arena.read([2])
    blk = host[arena.off[2]: arena.off[2] + out_words]
    assert not bool((blk.view(torch.int32) == NAN_BITS).any()), "an owned word was never written"
    got = blk.double().reshape(n, B, O2, e)
    lift = (rk[:, :, None] + (rk.conj() if cplx else rk)[:, None, :]).reshape(B, K2)
    want = []
    for f, v in enumerate((fullA + cst[None], lift + fullB)):
        if stages:
            v = _stage_ref(_stage_ref(v.reshape(B, Ki, Ki), w[wfold[f]]), w[wfold[f]]).reshape(B, O2)
        want.append(v)
    want = torch.stack(want)
    wre = want.real if cplx else want
    gre = got[..., 0]
    assert bool((gre[1, 0] == NEG_INF).all()) and not bool(torch.isnan(got[1, 0]).any())  # the all -inf row
    fin = torch.isfinite(wre)
    assert bool((gre[~fin] == wre[~fin]).all())
    err = (gre[fin] - wre[fin]).abs()
    assert bool((err <= 1e-4 * wre[fin].abs().clamp(min=1.0)).all()), float(err.max())
    if cplx:  # the phase, where the value is not a cancelled sum
        d = torch.remainder(got[..., 1] - want.imag + np.pi, 2 * np.pi) - np.pi
        assert float(d[fin].abs().max()) < 1e-3
