"""tests/layer_backward_restatement.py against torch autograd in fp64 (CPU only): on random finite inputs every restated
backward equals autograd through the corresponding forward -- written as the reference writes it: `logsumexp` of the prepared
inputs + log W, `Normal.log_prob`, advanced indexing of the table -- to 1e-12 of the largest entry of the gradient; at the
special points (whole -inf rows, zero weights, zero gout, marginalised x) it gives exactly the values its docstring states."""
import numpy as np
import pytest
import torch

import layer_backward_restatement as R

TOL = 1e-12
NEG_INF = float("-inf")


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _close(got, want):
    assert got.shape == want.shape and got.dtype == torch.float64
    assert float((got - want).abs().max()) <= TOL * float(want.abs().max()), float((got - want).abs().max() / want.abs().max())


def _layout(g, n_blocks, words, F, H, shared):
    """(arena size, row_off (F, H)): blocks `words` long with gaps between them, in shuffled order; `shared`: the folds draw
    their children from the n_blocks blocks with repeats, else every (fold, child) has a block of its own."""
    starts = (torch.randperm(n_blocks, generator=g) * (words + 3) + 2).numpy()
    pick = torch.randint(n_blocks, (F, H), generator=g).numpy() if shared else np.arange(F * H).reshape(F, H)
    return n_blocks * (words + 3) + 2, starts[pick]


def _sum_forward(arena, W, row_off, B, Ki, mode):
    """TorchSumLayer / TorchCPTLayer / TorchTuckerLayer under the lse-sum semiring: logsumexp_n(v[b, n] + log W[o, n])."""
    x = R.children(arena, row_off, B, Ki)
    F, H = x.shape[:2]
    if mode == R.PROD:
        v = x.sum(1)
    elif mode == R.CAT:
        v = x.permute(0, 2, 1, 3).reshape(F, B, H * Ki)
    else:
        v = x[:, 0]
        for h in range(1, H):
            v = (v.unsqueeze(-1) + x[:, h].unsqueeze(-2)).flatten(-2)
    return torch.logsumexp(v.unsqueeze(2) + torch.log(W).unsqueeze(1), -1)


SUM_CASES = [(R.CAT, 1, 5, 3), (R.CAT, 3, 4, 6), (R.PROD, 1, 6, 2), (R.PROD, 3, 7, 5), (R.KRON, 2, 3, 4), (R.KRON, 3, 2, 5), (R.KRON, 2, 4, 1)]


@pytest.mark.parametrize("accumulate", [0, 1, 2])
@pytest.mark.parametrize("mode,H,Ki,Ko", SUM_CASES)
def test_sum_lse(mode, H, Ki, Ko, accumulate):
    """Children shared between folds (and named twice by one fold) under accumulate = 2; a grad_row_off different from
    row_off under 0 and 1."""
    g = _g(10 * mode + H + accumulate)
    F, B = 3, 4
    N = Ki if mode == R.PROD else (H * Ki if mode == R.CAT else Ki ** H)
    shared = accumulate == 2
    size, row_off = _layout(g, 4 if shared else F * H, B * Ki, F, H, shared)
    arena = _randn(g, size) * 2
    W = torch.softmax(_randn(g, F, Ko, N), -1)
    leaves = [arena.clone().requires_grad_(True), W.clone().requires_grad_(True)]
    out = _sum_forward(*leaves, row_off, B, Ki, mode)
    gout = _randn(g, F, B, Ko)
    out.backward(gout)
    prior, dw_prior = _randn(g, size), _randn(g, F, Ko, N)
    if shared:
        got, dW = R.sum_lse_bwd(arena, prior, row_off, None, W, gout, dw_prior, B, Ki, mode, 2)
        _close(got, prior + leaves[0].grad)
    else:
        _, grow = _layout(g, F * H, B * Ki, F, H, False)
        got, dW = R.sum_lse_bwd(arena, prior, row_off, grow, W, gout, dw_prior, B, Ki, mode, accumulate)
        want = prior.clone()
        for f in range(F):
            for h in range(H):
                blk = leaves[0].grad[row_off[f, h]:row_off[f, h] + B * Ki]
                want[grow[f, h]:grow[f, h] + B * Ki] = blk + (prior[grow[f, h]:grow[f, h] + B * Ki] if accumulate else 0)
        _close(got, want)
    _close(dW, dw_prior + leaves[1].grad)


def test_sum_lse_special_points():
    """Row 0: every input -inf; row 1: gout = 0; output 0 has only zero weights; the last input unit has a zero column."""
    g = _g(3)
    F, H, B, Ki, Ko = 2, 2, 4, 3, 3
    for mode in (R.CAT, R.PROD, R.KRON):
        N = Ki if mode == R.PROD else (H * Ki if mode == R.CAT else Ki ** H)
        size, row_off = _layout(g, F * H, B * Ki, F, H, False)
        arena = _randn(g, size)
        x = R.children(arena, row_off, B, Ki).clone()
        for f in range(F):
            for h in range(H):
                arena[row_off[f, h]:row_off[f, h] + Ki] = NEG_INF
        W = torch.softmax(_randn(g, F, Ko, N), -1)
        W[:, 0] = 0.0
        W[:, :, N - 1] = 0.0
        gout = _randn(g, F, B, Ko)
        gout[:, 1] = 0.0
        G, dW = R.sum_lse_grads(arena, row_off, W, gout, B, Ki, mode)
        assert bool(torch.isfinite(G).all()) and bool(torch.isfinite(dW).all())
        assert bool((G[:, :, 0] == 0).all()) and bool((G[:, :, 1] == 0).all()), "an all -inf row / a gout = 0 row has gradient exactly 0"
        assert bool((dW[:, 0] == 0).all()) and bool((dW[:, :, N - 1] != 0).any()), "dW of a zero row is 0; a zero COLUMN still has dW"
        # rows 0 and 1 add nothing to dW: the same as the layer on rows 2, 3 alone
        arena2 = torch.zeros(size, dtype=torch.float64)
        ro2 = row_off.copy()
        for f in range(F):
            for h in range(H):
                arena2[row_off[f, h]:row_off[f, h] + 2 * Ki] = x[f, h, 2:].reshape(-1)
        _, dW2 = R.sum_lse_grads(arena2, ro2, W, gout[:, 2:].contiguous(), 2, Ki, mode)
        _close(dW, dW2)
        if mode == R.CAT:
            assert bool((G[:, H - 1, :, Ki - 1] == 0).all()), "the input unit of a zero column has gradient 0"


@pytest.mark.parametrize("accumulate", [0, 1, 2])
@pytest.mark.parametrize("H,K", [(1, 4), (2, 5), (3, 2)])
def test_mixing_lse(H, K, accumulate):
    g = _g(20 + H + accumulate)
    F, B = 3, 4
    shared = accumulate == 2
    size, row_off = _layout(g, 4 if shared else F * H, B * K, F, H, shared)
    arena = _randn(g, size) * 2
    mw = torch.softmax(_randn(g, F, K, H), -1)
    leaves = [arena.clone().requires_grad_(True), mw.clone().requires_grad_(True)]
    x = R.children(leaves[0], row_off, B, K)  # (F, H, B, K)
    out = torch.logsumexp(x + torch.log(leaves[1]).permute(0, 2, 1).unsqueeze(2), 1)
    gout = _randn(g, F, B, K)
    out.backward(gout)
    prior, dmw_prior = _randn(g, size), _randn(g, F, K, H)
    if shared:
        got, dmw = R.mixing_lse_bwd(arena, prior, row_off, None, mw, gout, dmw_prior, B, K, 2)
        _close(got, prior + leaves[0].grad)
    else:
        got, dmw = R.mixing_lse_bwd(arena, prior, row_off, None, mw, gout, dmw_prior, B, K, accumulate)
        own = torch.zeros(size, dtype=torch.bool)
        for o in row_off.reshape(-1):
            own[o:o + B * K] = True
        _close(got[own], leaves[0].grad[own] + (prior[own] if accumulate else 0))
        assert torch.equal(got[~own], prior[~own])
    _close(dmw, dmw_prior + leaves[1].grad)


def test_mixing_lse_special_points():
    """Row 0 all -inf with gout != 0, row 1 all -inf with gout = 0, row 2 finite with gout = 0; one coefficient exactly 0."""
    g = _g(4)
    F, H, B, K = 1, 2, 5, 3
    size, row_off = _layout(g, H, B * K, F, H, False)
    arena = _randn(g, size)
    for h in range(H):
        arena[row_off[0, h]:row_off[0, h] + 2 * K] = NEG_INF
    mw = torch.softmax(_randn(g, F, K, H), -1)
    mw[0, 1, 0] = 0.0
    gout = _randn(g, F, B, K)
    gout[0, 1:3] = 0.0
    G, dmw = R.mixing_lse_grads(arena, row_off, mw, gout, B, K)
    assert bool(torch.isfinite(G).all()) and bool(torch.isfinite(dmw).all())
    assert bool((G[:, :, :3] == 0).all()), "all -inf rows (with or without gout) and gout = 0 rows have gradient exactly 0"
    assert bool((G[0, 0, :, 1] == 0).all()) and float(dmw[0, 1, 0]) != 0.0, "a zero coefficient: no input gradient, but its own gradient"
    x = R.children(arena, row_off, B, K)
    arena2 = torch.zeros(size, dtype=torch.float64)
    for h in range(H):
        arena2[row_off[0, h]:row_off[0, h] + 2 * K] = x[0, h, 3:].reshape(-1)
    _, dmw2 = R.mixing_lse_grads(arena2, row_off, mw, gout[:, 3:].contiguous(), 2, K)
    _close(dmw, dmw2)  # (rows 0 .. 2 left dmw untouched)


@pytest.mark.parametrize("accumulate", [0, 1, 2])
def test_hadamard_and_kronecker(accumulate):
    g = _g(30 + accumulate)
    F, B = 3, 4
    shared = accumulate == 2
    for H, K in ((1, 3), (3, 4), (2, 3), (3, 2)):
        size, row_off = _layout(g, 4 if shared else F * H, B * K, F, H, shared)
        prior = _randn(g, size)
        for kron in ((False, True) if H >= 2 else (False,)):
            leaf = _randn(g, size).requires_grad_(True)
            x = R.children(leaf, row_off, B, K)
            if kron:
                out = x[:, 0]
                for h in range(1, H):
                    out = torch.flatten(out.unsqueeze(-1) + x[:, h].unsqueeze(-2), start_dim=-2)
            else:
                out = x.sum(dim=1)
            gout = _randn(g, *out.shape)
            out.backward(gout)
            got = R.kronecker_bwd(prior, row_off, gout, H, K, accumulate) if kron else R.hadamard_bwd(prior, row_off, gout, H, accumulate)
            own = torch.zeros(size, dtype=torch.bool)
            for o in row_off.reshape(-1):
                own[o:o + B * K] = True
            _close(got[own], leaf.grad[own] + (prior[own] if accumulate else 0))
            assert torch.equal(got[~own], prior[~own])
            if not kron and accumulate == 0:
                assert torch.equal(R.children(got, row_off, B, K), gout.unsqueeze(1).expand(F, H, B, K)), "a copy of gout"


@pytest.mark.parametrize("accumulate", [0, 1])
def test_categorical(accumulate):
    g = _g(40 + accumulate)
    F, B, K, C, V = 4, 9, 3, 5, 3
    xt = torch.randint(C, (V, B), generator=g, dtype=torch.int32)
    scope = np.array([2, 0, 2, 1])
    for gfold in (None, np.array([1, 0, 1, 2], dtype=np.int32)):
        table = _randn(g, F, C + 1, K).requires_grad_(True)
        x = xt[torch.as_tensor(scope)].long()  # (F, B)
        out = table[torch.arange(F).unsqueeze(1), x]  # (F, B, K)
        gblocks = _randn(g, F if gfold is None else 3, B, K)
        out.backward(gblocks if gfold is None else gblocks[torch.as_tensor(gfold).long()])
        prior = _randn(g, F, C + 1, K)
        got = R.categorical_bwd(gblocks, gfold, xt, scope, C, prior, accumulate)
        _close(got, table.grad + (prior if accumulate else 0))


def test_categorical_special_points():
    C, K = 3, 2
    xt = torch.tensor([[-1, 0, 3, 7, 2, -5]], dtype=torch.int32)
    gout = torch.arange(1.0, 13.0, dtype=torch.float64).view(1, 6, K)
    got = R.categorical_bwd(gout, None, xt, np.array([0]), C, None, 0)
    assert got.shape == (1, C + 1, K)
    assert torch.equal(got[0, C], gout[0, 0] + gout[0, 5]), "x < 0 goes to row C"
    assert torch.equal(got[0, C - 1], gout[0, 2] + gout[0, 3] + gout[0, 4]), "x >= C goes to row C - 1"
    assert torch.equal(got[0, 0], gout[0, 1]) and bool((got[0, 1] == 0).all())


def test_gaussian():
    g = _g(50)
    F, B, K, V = 4, 7, 3, 3
    xt = _randn(g, V, B) * 2
    scope = np.array([1, 0, 1, 2])
    mean, std = _randn(g, F, K).requires_grad_(True), (torch.rand(F, K, generator=g, dtype=torch.float64) + 0.2).requires_grad_(True)
    dist = torch.distributions.Normal(loc=mean.unsqueeze(1), scale=std.unsqueeze(1))
    out = dist.log_prob(xt[torch.as_tensor(scope)].unsqueeze(-1))  # (F, B, K)
    gout = _randn(g, F, B, K)
    out.backward(gout)
    dm, ds = R.gaussian_bwd(gout, xt, scope, mean.detach(), std.detach())
    _close(dm, mean.grad)
    _close(ds, std.grad)
    # marginalised rows contribute nothing: NaN in rows 2 and 5 of variable 1 == those rows' gout set to 0
    xn = xt.clone()
    xn[1, [2, 5]] = float("nan")
    g0 = gout.clone()
    g0[0, [2, 5]] = 0.0
    g0[2, [2, 5]] = 0.0
    dm2, ds2 = R.gaussian_bwd(gout, xn, scope, mean.detach(), std.detach())
    want = R.gaussian_bwd(g0, xt, scope, mean.detach(), std.detach())
    assert torch.equal(dm2, want[0]) and torch.equal(ds2, want[1])
    xn[0] = float("nan")
    dm3, ds3 = R.gaussian_bwd(gout, xn, scope, mean.detach(), std.detach())
    assert bool((dm3[1] == 0).all()) and bool((ds3[1] == 0).all()), "a variable marginalised in every row: exactly 0"


def test_segment_add_rows():
    g = _g(60)
    n = 5
    tmp = _randn(g, 6 * n)
    cptr, clist, coff = [0, 0, 1, 6], [3, 0, 5, 1, 2, 4], [2, 9, 16]
    prior = _randn(g, 24)
    got = R.segment_add_rows(tmp, cptr, clist, coff, prior, n)
    want = prior.clone()
    want[9:14] += tmp[15:20]
    for j in (0, 5, 1, 2, 4):
        want[16:21] += tmp[j * n:(j + 1) * n]
    assert torch.equal(got, want)
    assert torch.equal(got[2:7], prior[2:7]), "a child without entries keeps its prior"
