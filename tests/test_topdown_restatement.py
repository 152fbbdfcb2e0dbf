"""tests/topdown_restatement.py pinned to something independent, on the CPU: the flow messages of a layer, combined per child,
are torch autograd's gradient of sum_k f_k v_k with respect to the child log values; the derivative messages are the log of
autograd's gradient of the linear-space outputs contracted with exp(D); `stats_edge_sum` is w times autograd's gradient with
respect to w, summed over the live rows; the leaf restatements are their quotient / moment formulas evaluated entry by entry.
And the far-tail check of tests/test_gpu_topdown.py: on that family the plain fp32 run of the restatement is more than 4 x as far
from fp64 as the exact-shift fp32 run."""
import numpy as np
import pytest
import torch

import topdown_restatement as R

F64 = torch.float64
LAYERS = [(R.SUM, 0, 1, 4, 3), (R.SUM, 0, 3, 2, 4), (R.SUM, 1, 2, 3, 3), (R.CPT, 0, 2, 4, 3), (R.CPT, 0, 3, 3, 2), (R.TUCKER, 0, 2, 3, 4)]
B = 5


def _layer_outputs(case, kids, w, linear):
    """(F, B, Ko) outputs of the layer as a differentiable function of the child blocks `kids` (log values, or linear values
    with `linear`) and of w: v_k = log sum_i w[k, i] exp(e_i), or its exponential."""
    F, H, Ki, Ko, M = case.F, case.H, case.Ki, case.Ko, case.M
    cbase = case.cfolds[0]
    out = []
    for f in range(F):
        ins = [kids[int(case.child[f * H + h]) - cbase] for h in range(H)]
        if linear:
            ins = [torch.log(x) for x in ins]
        if case.type == R.SUM:
            e = torch.cat(ins, 1)
        elif case.type == R.CPT:
            e = sum(ins[1:], ins[0])
        else:
            e = (ins[0].unsqueeze(2) + ins[1].unsqueeze(1)).reshape(B, M)
        wf = w[f] if case.mask is None else w[f] * case.mask
        y = torch.exp(e) @ wf.t()
        out.append(y if linear else torch.log(y))
    return torch.stack(out)


def _case(type, diag, H, Ki, Ko, flow_pass, fam="normal", seed=0):
    g = torch.Generator().manual_seed(seed + 7 * type + H)
    return R.SumCase(type, diag, 3, H, Ki, Ko, B, fam, g, flow_pass=flow_pass)


def _args(c, vals=None):
    return (c.type, c.diag, c.child, c.w, c.F, c.H, c.Ki, c.Ko, c.M, c.vals if vals is None else vals, c.arena, c.val_off, c.fold_off, c.B)


def _vals64(c):
    """The value arena in fp64 with the parents' values unrounded (the case rounds them to fp32 once)."""
    vals = c.vals.double()
    kids = [R.block(vals, c.val_off, g, B, c.Ki) for g in c.cfolds]
    v = _layer_outputs(c, kids, c.w.double(), False)
    for j, p in enumerate(c.pfolds):
        R.block(vals, c.val_off, p, B, c.Ko).copy_(v[j])
    return vals


def _blocks(c, arena, folds, K):
    return torch.stack([R.block(arena, c.val_off, g, c.B, K) for g in folds])


@pytest.mark.parametrize("type,diag,H,Ki,Ko", LAYERS)
def test_flow_messages_are_the_gradient_of_the_weighted_log_values(type, diag, H, Ki, Ko):
    c = _case(type, diag, H, Ki, Ko, True)
    kids = [R.block(c.vals, c.val_off, g, B, Ki).double().clone().requires_grad_() for g in c.cfolds]
    f = _blocks(c, c.arena, c.pfolds, Ko).double()
    (f * _layer_outputs(c, kids, c.w.double(), False)).sum().backward()
    msg = R.flow_down_sum(*_args(c, _vals64(c)), F64)
    got = R.flow_segment_add(msg, *c.csr([1] * c.nc), c.arena, c.val_off, c.nc, Ki, B, F64)
    for g, k in zip(c.cfolds, kids):
        torch.testing.assert_close(R.block(got, c.val_off, g, B, Ki), k.grad, rtol=1e-10, atol=1e-14)
    # cfirst = 0: onto the prior
    onto = R.flow_segment_add(msg, *c.csr([0] * c.nc), c.arena, c.val_off, c.nc, Ki, B, F64)
    torch.testing.assert_close(_blocks(c, onto, c.cfolds, Ki), _blocks(c, got, c.cfolds, Ki) + _blocks(c, c.arena, c.cfolds, Ki).double(), rtol=1e-12,
                               atol=0)


@pytest.mark.parametrize("type,diag,H,Ki,Ko", LAYERS)
def test_derivative_messages_are_the_log_gradient_of_the_linear_outputs(type, diag, H, Ki, Ko):
    c = _case(type, diag, H, Ki, Ko, False)
    kids = [torch.exp(R.block(c.vals, c.val_off, g, B, Ki).double()).requires_grad_() for g in c.cfolds]
    D = _blocks(c, c.arena, c.pfolds, Ko).double()
    (torch.exp(D) * _layer_outputs(c, kids, c.w.double(), True)).sum().backward()
    msg = R.loo_down_sum(*_args(c, _vals64(c)), F64)
    got = R.loo_segment_lse(msg, *c.csr([1] * c.nc), c.arena, c.val_off, c.nc, Ki, B, F64)
    for g, k in zip(c.cfolds, kids):
        torch.testing.assert_close(R.block(got, c.val_off, g, B, Ki), torch.log(k.grad), rtol=1e-10, atol=1e-10)
    onto = R.loo_segment_lse(msg, *c.csr([0] * c.nc), c.arena, c.val_off, c.nc, Ki, B, F64)
    torch.testing.assert_close(_blocks(c, onto, c.cfolds, Ki), torch.logaddexp(_blocks(c, got, c.cfolds, Ki), _blocks(c, c.arena, c.cfolds, Ki).double()),
                               rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("type,diag,H,Ki,Ko", LAYERS)
def test_edge_statistics_are_w_times_the_gradient_in_w(type, diag, H, Ki, Ko):
    c = _case(type, diag, H, Ki, Ko, True)
    live = np.array([1, 0, 1, 1, 0], dtype=np.int32)
    kids = [R.block(c.vals, c.val_off, g, B, Ki).double() for g in c.cfolds]
    w = c.w.double().clone().requires_grad_()
    f = _blocks(c, c.arena, c.pfolds, Ko).double() * torch.as_tensor(live).view(1, B, 1)
    (f * _layer_outputs(c, kids, w, False)).sum().backward()
    prior = torch.randn(c.F, Ko, c.M, dtype=F64)
    got = R.stats_edge_sum(*_args(c, _vals64(c))[:-1], live, B, prior, F64)
    want = prior + c.w.double() * w.grad * (1 if c.mask is None else c.mask)
    torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-13)
    # the factored fp32 runs are the same function
    for dt in (torch.float32, R.EXACT32):
        torch.testing.assert_close(R.stats_edge_sum(*_args(c)[:-1], live, B, prior, dt).double(), want, rtol=1e-4, atol=1e-5)


def _product_case(type, H, Ki, flow_pass, seed=0):
    """Two consumers (global folds 0, 1; Ko units) over three child folds 2 .. 4: consumer 0 reads (2, 3[, 4]), consumer 1
    (3, 2[, 3]); returns (sizes / offsets, child, vals, arena, CSR with pairs (g, h))."""
    g = torch.Generator().manual_seed(seed + H + Ki)
    Ko = Ki if type == R.HADAMARD else Ki ** H
    child = np.array([[2, 3, 4][:H], [3, 2, 3][:H]], dtype=np.int32).reshape(-1)
    off, words = R.arena_offsets([B * Ko] * 2 + [B * Ki] * 3)
    vals, arena = torch.full((words,), float("nan")), torch.full((words,), float("nan"))
    for c in (2, 3, 4):
        R.block(vals, off, c, B, Ki).copy_(torch.randn(B, Ki, generator=g))
        R.block(arena, off, c, B, Ki).copy_(torch.rand(B, Ki, generator=g) if flow_pass else torch.randn(B, Ki, generator=g))
    for p in (0, 1):
        R.block(arena, off, p, B, Ko).copy_(torch.rand(B, Ko, generator=g) if flow_pass else torch.randn(B, Ko, generator=g))
    cstart, pairs = [0], []
    for c in (2, 3, 4):
        pairs += [(f, h) for f in range(2) for h in range(H) if child[f * H + h] == c]
        cstart.append(len(pairs))
    return off, child, vals, arena, np.array(cstart, dtype=np.int32), np.array([2, 3, 4], dtype=np.int32), pairs, Ko


def _product_outputs(type, H, Ki, child, kids):
    out = []
    for f in range(2):
        ins = [kids[int(child[f * H + h]) - 2] for h in range(H)]
        if type == R.HADAMARD:
            out.append(sum(ins[1:], ins[0]))
        else:
            v = ins[0]
            for x in ins[1:]:
                v = (v.unsqueeze(2) + x.unsqueeze(1)).reshape(B, -1)
            out.append(v)
    return out


@pytest.mark.parametrize("type,H,Ki", [(R.HADAMARD, 2, 4), (R.HADAMARD, 3, 3), (R.KRONECKER, 2, 3), (R.KRONECKER, 3, 2)])
def test_product_messages(type, H, Ki):
    off, child, vals, arena, cstart, cfold, pairs, Ko = _product_case(type, H, Ki, True)
    kids = [R.block(vals, off, c, B, Ki).double().clone().requires_grad_() for c in (2, 3, 4)]
    outs = _product_outputs(type, H, Ki, child, kids)
    sum((R.block(arena, off, f, B, Ko).double() * outs[f]).sum() for f in range(2)).backward()
    items = np.array([p[0] for p in pairs] if type == R.HADAMARD else [x for p in pairs for x in p], dtype=np.int32)
    first = np.array([1, 0, 1], dtype=np.int32)
    got = R.flow_down_product(type, cstart, cfold, first, items, arena, off, 3, H, Ki, Ko, B, F64)
    for j, c in enumerate((2, 3, 4)):
        if cstart[j + 1] == cstart[j]:
            continue
        want = kids[j].grad + (0 if first[j] else R.block(arena, off, c, B, Ki).double())
        torch.testing.assert_close(R.block(got, off, c, B, Ki), want, rtol=1e-12, atol=0)
    # the derivative pass: linear outputs prod_h u_h
    off, child, vals, arena, cstart, cfold, pairs, Ko = _product_case(type, H, Ki, False)
    kids = [torch.exp(R.block(vals, off, c, B, Ki).double()).requires_grad_() for c in (2, 3, 4)]
    outs = _product_outputs(type, H, Ki, child, [torch.log(k) for k in kids])
    sum((torch.exp(R.block(arena, off, f, B, Ko).double()) * torch.exp(outs[f])).sum() for f in range(2)).backward()
    items = np.array([x for p in pairs for x in p], dtype=np.int32)
    got = R.loo_down_product(type, cstart, cfold, first, items, child, 0, vals, arena, off, 3, H, Ki, Ko, B, F64)
    for j, c in enumerate((2, 3, 4)):
        if cstart[j + 1] == cstart[j]:
            continue
        want = torch.log(kids[j].grad)
        if not first[j]:
            want = torch.logaddexp(want, R.block(arena, off, c, B, Ki).double())
        torch.testing.assert_close(R.block(got, off, c, B, Ki), want, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------- leaves
def _leaf_case(seed=0):
    """Three input folds (global folds 0 .. 2 of K = 4, 3, 4 units and C = 5, 3, 5 states) over Q = 2 query variables: folds 0
    and 1 over variable 0, fold 2 over variable 1; fold 3 (one unit) is the root."""
    g = torch.Generator().manual_seed(seed)
    Ks, Cs = [4, 3, 4], [5, 3, 5]
    off, words = R.arena_offsets([B * k for k in Ks] + [B])
    toff = np.cumsum([0] + [k * c for k, c in zip(Ks, Cs)])
    zoff = np.cumsum([0] + Ks)
    entries = np.array([[s, Ks[s], Cs[s], toff[s], zoff[s]] for s in range(3)], dtype=np.int64)
    ntab = torch.cat([torch.softmax(torch.randn(k, c, generator=g), -1).reshape(-1) for k, c in zip(Ks, Cs)])
    lz = torch.randn(int(zoff[-1]), generator=g)
    lz[1] = R.NEG_INF
    flow, der, vals = (torch.full((words,), float("nan")) for _ in range(3))
    for s in range(3):
        R.block(flow, off, s, B, Ks[s]).copy_(torch.rand(B, Ks[s], generator=g))
        d = torch.randn(B, Ks[s], generator=g) * 3
        d[torch.rand(B, Ks[s], generator=g) < 0.2] = R.NEG_INF
        R.block(der, off, s, B, Ks[s]).copy_(d)
        R.block(vals, off, s, B, Ks[s]).copy_(torch.randn(B, Ks[s], generator=g))
    der[off[2]:off[2] + 4] = R.NEG_INF  # (row 0 of variable 1: no derivative at all)
    R.block(vals, off, 3, B, 1).copy_(torch.tensor([[-3.0], [R.NEG_INF], [-1.0], [-2.0], [-5.0]]))
    bad = np.array([0, 0, 0, 1, 0], dtype=np.int32)
    return off, entries, np.array([0, 2, 3], dtype=np.int32), ntab, lz, flow, der, vals, bad, Ks, Cs


def test_flow_leaves_are_the_moment_formulas():
    off, entries, qstart, ntab, lz, flow, der, vals, bad, Ks, Cs = _leaf_case()
    out, logev = R.flow_leaf_categorical(entries[:, :4], qstart, 2, 5, ntab, flow, vals, off, 3, 1, bad, B, F64)
    mean, std = torch.randn(11, dtype=F64), torch.rand(11, dtype=F64) + 0.1
    gent = entries[:, :4].copy()
    gent[:, 3] = entries[:, 4]
    gout, _ = R.flow_leaf_gaussian(gent, qstart, 2, mean, std, flow, vals, off, 3, 1, bad, B, F64)
    for n in range(B):
        dead = n in (1, 3)
        assert torch.isnan(logev[n]) == (n == 3) and (n == 3 or logev[n] == vals[off[3] + n].double())
        for q in range(2):
            s1 = s2 = 0.0
            for c in range(5):
                want = 0.0
                for s in range(qstart[q], qstart[q + 1]):
                    for k in range(Ks[s]):
                        if c < Cs[s]:
                            want += float(flow[off[s] + n * Ks[s] + k]) * float(ntab[entries[s, 3] + k * Cs[s] + c])
                assert (torch.isnan(out[n, q, c]) if dead else abs(float(out[n, q, c]) - want) < 1e-12)
            for s in range(qstart[q], qstart[q + 1]):
                for k in range(Ks[s]):
                    fk, mu, sd = float(flow[off[s] + n * Ks[s] + k]), float(mean[entries[s, 4] + k]), float(std[entries[s, 4] + k])
                    s1 += fk * mu
                    s2 += fk * (sd * sd + mu * mu)
            if dead:
                assert bool(torch.isnan(gout[n, q]).all())
            else:
                assert abs(float(gout[n, q, 0]) - s1) < 1e-12 and abs(float(gout[n, q, 1]) - (s2 - s1 * s1)) < 1e-12


def test_derivative_leaves_are_the_quotient_formulas():
    off, entries, qstart, ntab, lz, flow, der, vals, bad, Ks, Cs = _leaf_case()
    out = R.loo_leaf_categorical(entries, qstart, 2, 5, ntab, lz, der, off, bad, B, F64)
    mean, std = torch.randn(11, dtype=F64), torch.rand(11, dtype=F64) + 0.1
    gent = entries.copy()
    gent[:, 3] = entries[:, 4]
    gout = R.loo_leaf_gaussian(gent, qstart, 2, mean, std, der, off, bad, B, F64)
    ev = torch.tensor([[0, 1], [-1, 2], [4, 0], [1, 1], [2, -1]], dtype=torch.int64)
    lp = R.loo_log_probs(entries, qstart, np.array([0, 0], dtype=np.int32), 2, lz, der, vals, off, ev, 0, bad, B, F64)
    for n in range(B):
        for q in range(2):
            units = [(s, k) for s in range(qstart[q], qstart[q + 1]) for k in range(Ks[s])]
            d = np.array([float(der[off[s] + n * Ks[s] + k]) for s, k in units])
            z = np.array([float(lz[entries[s, 4] + k]) for s, k in units])
            v = np.array([float(vals[off[s] + n * Ks[s] + k]) for s, k in units])
            a = np.zeros(5)
            for (s, k), dk, zk in zip(units, d, z):
                for c in range(Cs[s]):
                    a[c] += np.exp(dk + zk) * float(ntab[entries[s, 3] + k * Cs[s] + c])
            pi = np.exp(d)
            mu = np.array([float(mean[entries[s, 4] + k]) for s, k in units])
            sd = np.array([float(std[entries[s, 4] + k]) for s, k in units])
            if n == 3 or a.sum() == 0:
                assert bool(torch.isnan(out[n, q]).all())
            else:
                np.testing.assert_allclose(out[n, q].numpy(), a / a.sum(), rtol=1e-12, atol=1e-15)
            if n == 3 or pi.sum() == 0:
                assert bool(torch.isnan(gout[n, q]).all())
            else:
                s1, s2 = (pi * mu).sum() / pi.sum(), (pi * (sd * sd + mu * mu)).sum() / pi.sum()
                np.testing.assert_allclose(gout[n, q].numpy(), [s1, s2 - s1 * s1], rtol=1e-10, atol=1e-12)
            if n == 3 or (ev[n, q] >= 0 and np.exp(d + z).sum() == 0):
                assert torch.isnan(lp[n, q])
            elif ev[n, q] < 0:
                assert lp[n, q] == 0
            else:
                np.testing.assert_allclose(float(lp[n, q]), np.log(np.exp(d + v).sum()) - np.log(np.exp(d + z).sum()), rtol=1e-10, atol=1e-12)
    assert bool(torch.isnan(out[0, 1]).all()) and bool(torch.isnan(lp[0, 1]))  # (the row of variable 1 without a derivative)


def test_check_evidence_and_the_statistics_of_the_leaves():
    g = torch.Generator().manual_seed(3)
    states = np.array([3, 0, 5], dtype=np.int32)
    ev = torch.tensor([[0, 9, 4], [3, -1, -2], [-1, 2, 5], [2, 0, 0], [1, 1, 7]], dtype=torch.int64)
    clean, bad, flag = R.flow_check_evidence(ev, 0, states, B, 3)
    assert bad.tolist() == [0, 1, 1, 0, 1] and flag == 1
    assert clean.tolist() == [[0, 9, 4], [0, -1, -2], [-1, 2, 0], [2, 0, 0], [1, 1, 0]]
    evf = ev.float()
    evf[1, 1] = float("nan")
    cleanf, badf, _ = R.flow_check_evidence(evf, 1, states, B, 3)
    assert badf.tolist() == bad.tolist() and torch.equal(torch.nan_to_num(cleanf, nan=-1.0), clean.float().clamp(min=-2))
    # statistics: folds over variables 2 and 0, K = 3 units, C = 4 states (an observed 4 of variable 2 is beyond C)
    F, K, C = 2, 3, 4
    off, words = R.arena_offsets([B * K] * F + [B * 2])
    flow = torch.rand(words, generator=g)
    scope = np.array([2, 0], dtype=np.int64)
    ntab = torch.softmax(torch.randn(F, K, C, generator=g), -1)
    live = np.array([1, 1, 0, 1, 1], dtype=np.int32)
    prior = torch.randn(F, K, C, dtype=F64)
    got = R.stats_leaf_categorical(scope, ntab, F, K, C, ev, 0, 3, flow, off, 0, live, B, prior, F64)
    want = prior.clone()
    for f in range(F):
        for n in range(B):
            if not live[n]:
                continue
            x = int(ev[n, scope[f]])
            for k in range(K):
                fk = float(flow[off[f] + n * K + k])
                if x < 0:
                    want[f, k] += fk * ntab[f, k].double()
                elif x < C:
                    want[f, k, x] += fk
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-14)
    gotf = R.stats_leaf_categorical(scope, ntab, F, K, C, ev.float() + 0.5 * (ev >= 0), 1, 3, flow, off, 0, live, B, prior, F64)
    torch.testing.assert_close(gotf, want, rtol=1e-12, atol=1e-14)  # (a float batch is truncated)
    x = torch.randn(B, 3, generator=g)
    x[0, 2] = float("nan")
    mean, std = torch.randn(F, K, generator=g), torch.rand(F, K, generator=g) + 0.1
    gp = torch.randn(F, K, 3, dtype=F64)
    gg = R.stats_leaf_gaussian(scope, mean, std, F, K, x, 3, flow, off, 0, live, B, gp, F64)
    for f in range(F):
        for k in range(K):
            s = np.zeros(3)
            for n in range(B):
                if live[n]:
                    fk, xv = float(flow[off[f] + n * K + k]), float(x[n, scope[f]])
                    m1, m2 = (xv, xv * xv) if xv == xv else (float(mean[f, k]), float(std[f, k]) ** 2 + float(mean[f, k]) ** 2)
                    s += fk * np.array([1.0, m1, m2])
            np.testing.assert_allclose(gg[f, k].numpy(), gp[f, k].numpy() + s, rtol=1e-12)
    fold_ko, unit_off = np.array([K, K, 2], dtype=np.int32), np.array([5, 0, 9], dtype=np.int64)
    up = torch.randn(12, dtype=F64)
    gu = R.stats_unit_sum(flow, off, fold_ko, unit_off, 3, live, B, up, F64)
    for gf in range(3):
        for k in range(int(fold_ko[gf])):
            want_u = float(up[unit_off[gf] + k]) + sum(float(flow[off[gf] + n * int(fold_ko[gf]) + k]) for n in range(B) if live[n])
            assert abs(float(gu[unit_off[gf] + k]) - want_u) < 1e-12
    assert float(gu[8]) == float(up[8]) and float(gu[11]) == float(up[11])


# ------------------------------------------------------------------------------------------------ the far-tail yardstick
@pytest.mark.parametrize("type,diag,H,Ki,Ko", LAYERS + [(R.SUM, 0, 1, 32, 32), (R.CPT, 0, 2, 32, 64)])
def test_far_tail_inputs_are_far_enough_out(type, diag, H, Ki, Ko):
    """On the far-tail family the plain fp32 run (log f - v rounded at the size of v) is more than 4 x as far from fp64 as the
    exact-shift fp32 run, for the flow messages and for the edge statistics: a kernel that rounds the exponents it promises not
    to round stands above 4 x the exact-shift yardstick."""
    c = _case(type, diag, H, Ki, Ko, True, "far-tail", seed=1)
    live = np.ones(B, dtype=np.int32)
    prior = torch.zeros(c.F, Ko, c.M)
    for name, run in (("messages", lambda dt: R.flow_down_sum(*_args(c), dt)), ("edge", lambda dt: R.stats_edge_sum(*_args(c)[:-1], live, B, prior, dt))):
        ref = run(F64)
        pos = ref > 0
        plain, exact = (((run(dt).double() - ref).abs() / ref.abs().clamp_min(1e-300))[pos].max().item() for dt in (torch.float32, R.EXACT32))
        print(f"far-tail {name}: plain {plain:.3e} exact-shift {exact:.3e}")
        assert plain > 4 * exact, f"{name}: plain fp32 {plain:.3e} within 4 x exact-shift fp32 {exact:.3e}: the inputs are not far enough out"
        assert exact < 4e-6
