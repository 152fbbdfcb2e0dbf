"""tests/jobs_restatement.py pinned to torch autograd in fp64, through the plain formula of every layer: `logsumexp` over a
log-space product (the sum jobs and the root), the mixing sum, `log_softmax(theta)[:, x]`, `Normal.log_prob`, and the composite of a
sum job under a mixing fold with `mix_out` at its exact value.  Loss = sum(G * out); agreement 1e-12 relative to max|row|.  The
conventions autograd does not have (an out-of-range category, a -inf row, a coefficient of exactly 0) are pinned by value."""
import pytest
import torch

import jobs_restatement as J

TOL = 1e-12
NEG_INF = float("-inf")


def _close(got, want, what):
    assert got.shape == want.shape, what
    scale = want.abs().amax(dim=-1, keepdim=True) if want.dim() else want.abs()
    scale = torch.where(scale > 0, scale, torch.ones_like(scale))
    err = float(((got - want).abs() / scale).max())
    assert err <= TOL, f"{what}: {err:.3e}"


def _leaf(*shape, g):
    return torch.randn(*shape, generator=g, dtype=torch.float64).requires_grad_(True)


def _sum_formula(v, W):
    """out[b, o] = logsumexp_n(log W[o, n] + v[b, n])."""
    return torch.logsumexp(torch.log(W).unsqueeze(0) + v.unsqueeze(1), dim=-1)


@pytest.mark.parametrize("n_in,n_g", [(1, 1), (3, 2)])
def test_sum_job(n_in, n_g):
    g = torch.Generator().manual_seed(n_in)
    B = 7
    blocks = [_leaf(B, 64, g=g) for _ in range(n_in)]
    theta = _leaf(64, 64, g=g)
    Wl = torch.softmax(theta, -1)
    Wl.retain_grad()
    glist = [torch.randn(B, 64, generator=g, dtype=torch.float64) for _ in range(n_g)]
    out = _sum_formula(sum(blocks), Wl)
    (sum(glist) * out).sum().backward()
    W = Wl.detach()
    _close(J.sum_job_fwd([b.detach() for b in blocks], W), out.detach(), "out")
    for mode, want in ((0, Wl.grad), (1, theta.grad)):
        gx, dth, _ = J.sum_job_bwd([b.detach() for b in blocks], W, glist, mode)
        _close(dth, want, f"dtheta mode {mode}")
        for b in blocks:
            _close(gx, b.grad, "gx")


def test_sum_job_gathers_table_rows():
    g = torch.Generator().manual_seed(3)
    C, B = 5, 9
    table = _leaf(C + 1, 64, g=g)
    W = torch.softmax(torch.randn(64, 64, generator=g, dtype=torch.float64), -1)
    x = torch.tensor([0, 4, -1, 2, 7, 5, 1, -3, 4], dtype=torch.int32)
    rows = torch.tensor([0, 4, 5, 2, 4, 4, 1, 5, 4])  # -1 / -3 -> row C, 7 / 5 (>= C) -> row C - 1
    assert torch.equal(J.input_rows(x, C), rows)
    out = _sum_formula(table[rows], W)
    G = torch.randn(B, 64, generator=g, dtype=torch.float64)
    (G * out).sum().backward()
    _close(J.sum_job_fwd(None, W, x, table.detach()), out.detach(), "out")
    gx, _, _ = J.sum_job_bwd(None, W, [G], 0, x, table.detach())
    _close(torch.zeros(C + 1, 64, dtype=torch.float64).index_add_(0, rows, gx), table.grad, "gx scattered over the table rows")


def test_neginf_rows_and_zero_gradients():
    g = torch.Generator().manual_seed(4)
    v = torch.randn(4, 64, generator=g, dtype=torch.float64)
    v[1] = NEG_INF
    v[2, ::2] = NEG_INF
    W = torch.softmax(torch.randn(64, 64, generator=g, dtype=torch.float64), -1)
    G = torch.randn(4, 64, generator=g, dtype=torch.float64)
    G[3] = 0.0
    out = J.sum_job_fwd([v], W)
    assert bool((out[1] == NEG_INF).all()) and bool(torch.isfinite(out[[0, 2, 3]]).all())
    gx, dth, _ = J.sum_job_bwd([v], W, [G], 1)
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(dth).all())
    assert bool((gx[1] == 0).all()) and bool((gx[3] == 0).all()) and bool((gx[2, ::2] == 0).all())
    keep = [0, 2]
    _, dth2, _ = J.sum_job_bwd([v[keep]], W, [G[keep]], 1)
    _close(dth, dth2, "a -inf row and a zero-gradient row add nothing to dtheta")
    w = torch.softmax(torch.randn(64, 3, generator=g, dtype=torch.float64), -1)
    slots = [[v], [v.clone()], [v.clone()]]
    assert bool((J.mix_job_fwd(slots, w)[1] == NEG_INF).all())
    gxm, dm = J.mix_job_bwd(slots, w, [G], 1)
    assert bool(torch.isfinite(gxm).all()) and bool(torch.isfinite(dm).all()) and bool((gxm[:, 1] == 0).all())
    o, ll, gr, dw, dc = J.root([[v]], W[:1], None, 1, seed_const=-0.25)
    assert float(o[1]) == NEG_INF and bool((gr[0, 1] == 0).all()) and bool(torch.isfinite(dw).all()) and dc is None


@pytest.mark.parametrize("H,S", [(1, 1), (3, 2), (5, 1)])
def test_mix_job(H, S):
    g = torch.Generator().manual_seed(10 * H + S)
    B = 6
    slots = [[_leaf(B, 64, g=g) for _ in range(S)] for _ in range(H)]
    theta = _leaf(64, H, g=g)
    wl = torch.softmax(theta, -1)
    wl.retain_grad()
    G = torch.randn(B, 64, generator=g, dtype=torch.float64)
    x = torch.stack([sum(s) for s in slots])  # (H, B, 64)
    out = torch.logsumexp(torch.log(wl).t().unsqueeze(1) + x, dim=0)
    (G * out).sum().backward()
    det = [[b.detach() for b in s] for s in slots]
    _close(J.mix_job_fwd(det, wl.detach()), out.detach(), "out")
    for mode, want in ((0, wl.grad), (1, theta.grad)):
        gx, dth = J.mix_job_bwd(det, wl.detach(), [G], mode)
        _close(dth, want, f"dtheta mode {mode}")
        _close(J.mix_params(wl.grad, wl.detach(), mode), want, f"mix_params mode {mode}")
        for h in range(H):
            _close(gx[h], slots[h][0].grad, "gx")


@pytest.mark.parametrize("h,n_partner", [(0, 0), (2, 2)])
def test_sum_job_under_a_mixing_fold(h, n_partner):
    """The composite: a mixing fold of H slots whose slot h is this sum job's output plus its partners; `mix_out` exact."""
    g = torch.Generator().manual_seed(20 + h)
    B, H = 5, 3
    v = _leaf(B, 64, g=g)
    theta = _leaf(64, 64, g=g)
    partners = [torch.randn(B, 64, generator=g, dtype=torch.float64) for _ in range(n_partner)]
    others = [torch.randn(B, 64, generator=g, dtype=torch.float64) for _ in range(H)]
    mtheta = _leaf(64, H, g=g)
    mw = torch.softmax(mtheta, -1)
    mw.retain_grad()
    W = torch.softmax(theta, -1)
    xh = _sum_formula(v, W) + sum(partners) if partners else _sum_formula(v, W)
    x = torch.stack([xh if k == h else others[k] for k in range(H)])
    mix_out = torch.logsumexp(torch.log(mw).t().unsqueeze(1) + x, dim=0)
    G = torch.randn(B, 64, generator=g, dtype=torch.float64)
    (G * mix_out).sum().backward()
    gx, dth, col = J.sum_job_bwd([v.detach()], W.detach(), [G], 1, mix_out=mix_out.detach(), mix_w=mw.detach(), mix_h=h, partners=partners)
    _close(gx, v.grad, "gx")
    _close(dth, theta.grad, "dtheta")
    _close(col, mw.grad[:, h], "mix_dw column")
    mw0 = mw.detach().clone()
    mw0[3, h] = 0.0
    col0 = J.sum_job_bwd([v.detach()], W.detach(), [G], 1, mix_out=mix_out.detach(), mix_w=mw0, mix_h=h, partners=partners)[2]
    assert float(col0[3]) == 0.0 and bool(torch.isfinite(col0).all()), "a coefficient of exactly 0 gives mix_dw = 0"


def test_nsum_adds_in_list_order():
    a, b, c = torch.tensor([1e8]), torch.tensor([1.0]), torch.tensor([-1e8])
    assert float(J.nsum([a, b, c])) == 0.0 and float(J.nsum([a, c, b])) == 1.0  # fp32: (1e8 + 1) - 1e8 = 0


@pytest.mark.parametrize("R,S,with_c,seeded", [(1, 1, False, False), (1, 2, True, True), (4, 3, True, False), (5, 1, True, True)])
def test_root(R, S, with_c, seeded):
    g = torch.Generator().manual_seed(R * 10 + S)
    B = 6
    folds = [[_leaf(B, 64, g=g) for _ in range(S)] for _ in range(R)]
    theta = _leaf(R, 64, g=g)
    W = torch.softmax(theta, -1)
    W.retain_grad()
    tc = _leaf(R, g=g)
    c = torch.softmax(tc, -1)
    c.retain_grad()
    o = torch.stack([torch.logsumexp(torch.log(W[r]) + sum(folds[r]), dim=-1) for r in range(R)])  # (R, B)
    out = torch.logsumexp(torch.log(c).unsqueeze(1) + o, dim=0) if with_c else o[0]
    seed = torch.randn(B, generator=g, dtype=torch.float64) if seeded else torch.full((B,), -1.0 / B, dtype=torch.float64)
    (seed * out).sum().backward()
    det = [[b.detach() for b in f] for f in folds]
    kw = {"seed": seed} if seeded else {"seed_const": -1.0 / B}
    for mode, want_w, want_c in ((0, W.grad, c.grad), (1, theta.grad, tc.grad)):
        got, ll, gx, dw, dc = J.root(det, W.detach(), c.detach() if with_c else None, mode, **kw)
        _close(got, out.detach(), "out")
        assert float(ll[1]) == B
        _close(ll[0], out.detach().sum(), "ll")
        _close(dw, want_w, f"dtheta_w mode {mode}")
        if with_c:
            _close(dc, want_c, f"dtheta_c mode {mode}")
        else:
            assert dc is None
        for r in range(R):
            _close(gx[r], folds[r][0].grad, "gx")
    bad = J.root(det, W.detach(), c.detach() if with_c else None, 1, bad=True, **kw)
    assert bool(torch.isnan(bad[0]).all()) and bool(torch.isnan(bad[1][0])) and torch.equal(bad[3], dw)


@pytest.mark.parametrize("C", [1, 2, 7])
def test_cat_job(C):
    g = torch.Generator().manual_seed(C)
    B = 40
    theta = _leaf(64, C, g=g)
    x = torch.randint(-1, C, (B,), generator=g).to(torch.int32)
    x[0] = C - 1
    G = torch.randn(B, 64, generator=g, dtype=torch.float64)
    lp = torch.log_softmax(theta, -1)  # (64, C)
    live = x >= 0
    out = lp[:, x[live].long()].t()  # (rows, 64); a marginalised row reads the integral row of zeros: no gradient
    (G[live] * out).sum().backward()
    _close(J.cat_job_bwd(G, x, theta.detach()), theta.grad, "dtheta")
    table = torch.zeros(C + 1, 64, dtype=torch.float64)
    table[:C] = lp.detach().t()
    _close(J.cat_job_bwd(G, x, theta.detach(), table), theta.grad, "dtheta from the table")
    xo = x.clone()
    xo[0] = C + 5  # out of range: row C - 1
    _close(J.cat_job_bwd(G, xo, theta.detach()), theta.grad, "an out-of-range category selects row C - 1")


@pytest.mark.parametrize("has_ss", [False, True])
def test_gauss_job(has_ss):
    g = torch.Generator().manual_seed(30 + has_ss)
    B, vmin, vmax = 33, 0.1, 2.5
    mean = _leaf(64, g=g)
    th = _leaf(64, g=g)
    sd = vmin + (vmax - vmin) * torch.sigmoid(th) if has_ss else th.abs() + 0.2
    sd.retain_grad()
    x = torch.randn(B, generator=g, dtype=torch.float64)
    x[::5] = float("nan")
    live = ~torch.isnan(x)
    G = torch.randn(B, 64, generator=g, dtype=torch.float64)
    out = torch.distributions.Normal(mean, sd).log_prob(x[live].unsqueeze(-1))
    (G[live] * out).sum().backward()
    dm, ds = J.gauss_job_bwd(G, x, mean.detach(), sd.detach(), vmin, vmax, has_ss)
    _close(dm, mean.grad, "dmean")
    _close(ds, th.grad if has_ss else sd.grad, "dsd")
