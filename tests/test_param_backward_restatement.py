"""tests/param_backward_restatement.py against torch autograd in fp64 (CPU only): on random inputs away from the special points
every restated backward equals autograd through the corresponding forward to 1e-12 of the largest entry of the gradient; at
the special points it gives exactly the values its docstring states."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import param_backward_restatement as R
from cirkit_amd.plan import IDX_NONE, FoldIndex, ParamGraph, ParamNode
from oracle.torch_oracle import eval_param

TOL = 1e-12
INF = float("inf")


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _close(got, want):
    assert got.shape == want.shape and got.dtype == torch.float64
    assert float((got - want).abs().max()) <= TOL * float(want.abs().max()), float((got - want).abs().max() / want.abs().max())


def _grad(fn, *xs):
    """(value, gradients) of sum(fn(*leaves) * dout) for a fixed random dout."""
    leaves = [x.clone().requires_grad_(True) for x in xs]
    y = fn(*leaves)
    dout = _randn(_g(99), *y.shape)
    y.backward(dout)
    return y.detach(), dout, [l.grad for l in leaves]


def _node_graph(op, config, shapes, out_shape, Fo):
    nodes = [ParamNode("tensor", Fo, tuple(sh), {"tensor": f"t{i}"}, []) for i, sh in enumerate(shapes)]
    nodes.append(ParamNode(op, Fo, tuple(out_shape), dict(config), [FoldIndex([i], IDX_NONE) for i in range(len(shapes))]))
    return ParamGraph(nodes, FoldIndex([len(nodes) - 1], IDX_NONE), Fo, tuple(out_shape))


@pytest.mark.parametrize("accumulate", [False, True])
def test_softmax_rows_and_strided(accumulate):
    g = _g(1)
    x = _randn(g, 7, 33)
    prior = _randn(g, 7, 33) if accumulate else None
    y, dout, (gx,) = _grad(lambda t: torch.softmax(t, -1), x)
    _close(R.softmax_bwd_rows(y, dout, prior), gx + (prior if accumulate else 0))
    x = _randn(g, 3, 6, 5)
    prior = _randn(g, 3, 6, 5) if accumulate else None
    for log_space, fwd in ((0, torch.softmax), (1, torch.log_softmax)):
        y, dout, (gx,) = _grad(lambda t: fwd(t, 1), x)
        _close(R.softmax_bwd_strided(y, dout, log_space, prior), gx + (prior if accumulate else 0))


def test_log_softmax_where_y_is_minus_inf():
    y = torch.log_softmax(torch.tensor([[[0.5], [-INF], [1.0]]], dtype=torch.float64), 1)
    dy = torch.tensor([[[2.0], [3.0], [-1.0]]], dtype=torch.float64)
    assert float(R.softmax_bwd_strided(y, dy, 1)[0, 1, 0]) == 3.0  # dx = dy there


@pytest.mark.parametrize("op", R.UNARY_OPS)
def test_unary(op):
    g = _g(2)
    x = _randn(g, 5, 40) * 3
    kw = {}
    if op == "log":
        x = x.abs() + 0.1
    fwd = {"sigmoid": torch.sigmoid, "exp": torch.exp, "log": torch.log, "square": torch.square, "softplus": F.softplus,
           "clamp": lambda t: torch.clamp(t, min=-0.5, max=0.25)}[op]
    if op == "clamp":
        kw = {"vmin": -0.5, "vmax": 0.25}
    if op == "softplus":
        x[0, :4] = torch.tensor([19.5, 20.5, -30.0, 25.0], dtype=torch.float64)
    y, dout, (gx,) = _grad(fwd, x)
    _close(R.unary_bwd(op, x, y, dout, **kw), gx)
    prior = _randn(g, 5, 40)
    _close(R.unary_bwd(op, x, y, dout, prior, **kw), gx + prior)


def test_unary_special_points():
    t = lambda *v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    got = R.unary_bwd("log", t(0.0, 0.0, 0.0, 2.0), torch.log(t(0.0, 0.0, 0.0, 2.0)), t(0.0, 2.0, -3.0, 0.0))
    assert got.tolist() == [0.0, INF, -INF, 0.0]
    x = t(-0.5, 0.25, np.nextafter(-0.5, -1.0), np.nextafter(0.25, 1.0), 0.0)
    got = R.unary_bwd("clamp", x, torch.clamp(x, -0.5, 0.25), t(1.5, 1.5, 1.5, 1.5, 1.5), vmin=-0.5, vmax=0.25)
    assert got.tolist() == [1.5, 1.5, 0.0, 0.0, 1.5]
    got = R.unary_bwd("clamp", t(-3.0, 5.0), t(1e-18, 5.0), t(2.0, 2.0), vmin=1e-18)  # (an absent bound is open)
    assert got.tolist() == [0.0, 2.0]
    x = t(20.0, 20.5)
    got = R.unary_bwd("softplus", x, F.softplus(x), t(1.0, 1.0))
    assert got[1] == 1.0 and got[0] == 1 / (1 + math.exp(-20.0))  # (at the threshold itself the smooth branch: torch's x > 20)
    # ... and torch agrees on both sides
    xs = x.clone().requires_grad_(True)
    F.softplus(xs).sum().backward()
    assert float((xs.grad - got).abs().max()) <= TOL
    assert R.unary_bwd("sigmoid", t(40.0), t(1.0), t(3.0)).tolist() == [0.0]  # (saturated: y == 1)
    for op in R.UNARY_OPS:  # dy == 0: exactly 0, and the prior comes back untouched
        assert R.unary_bwd(op, t(0.0), t(0.0), t(0.0), t(7.0)).tolist() == [7.0]


@pytest.mark.parametrize("vmin,vmax", [(0.0, 1.0), (1e-4, 10.0), (-2.0, -0.5)])
def test_scaled_sigmoid(vmin, vmax):
    g = _g(3)
    x = _randn(g, 4, 9) * 2
    y, dout, (gx,) = _grad(lambda t: torch.sigmoid(t) * (vmax - vmin) + vmin, x)
    _close(R.scaled_sigmoid_bwd(y, dout, vmin, vmax), gx)
    prior = _randn(g, 4, 9)
    _close(R.scaled_sigmoid_bwd(y, dout, vmin, vmax, prior), gx + prior)
    edge = R.scaled_sigmoid_bwd(torch.tensor([vmin, vmax], dtype=torch.float64), torch.tensor([5.0, -5.0], dtype=torch.float64), vmin, vmax)
    assert edge.tolist() == [0.0, 0.0]


@pytest.mark.parametrize("Fo,K,H", [(1, 1, 1), (3, 5, 2), (2, 7, 9)])
def test_mixing_weight(Fo, K, H):
    g = _g(4)
    x = _randn(g, Fo, K, H)
    graph = _node_graph("mixing_weight", {}, [(K, H)], (K, H * K), Fo)
    y, dout, (gx,) = _grad(lambda t: eval_param(graph, {"t0": t}), x)
    assert tuple(y.shape) == (Fo, K, H * K)
    assert torch.equal(R.mixing_weight_bwd(dout, K, H), gx)  # (a pick: exact)
    prior = _randn(g, Fo, K, H)
    assert torch.equal(R.mixing_weight_bwd(dout, K, H, prior), prior + gx)
    # nothing off the block diagonal is read
    poisoned = torch.full_like(dout, float("nan")).reshape(Fo, K, H, K)
    for k in range(K):
        poisoned[:, k, :, k] = dout.reshape(Fo, K, H, K)[:, k, :, k]
    assert torch.equal(R.mixing_weight_bwd(poisoned.reshape(Fo, K, H * K), K, H), gx)


def test_scatter_add_and_axpy():
    g = _g(5)
    src, dst = _randn(g, 6, 11), _randn(g, 4, 11)
    idx = torch.tensor([2, 0, 2, 2, 3, 0])
    _close(R.scatter_add_folds(src, idx, dst), dst.index_add(0, idx, src))  # (torch's index_add: what the kernel does)
    assert torch.equal(R.scatter_add_folds(src, idx, dst)[1], dst[1])  # (a fold nobody hits)
    # the gather x[idx] has this scatter as its backward
    x = _randn(g, 4, 11)
    _, dout, (gx,) = _grad(lambda t: t[idx], x)
    _close(R.scatter_add_folds(dout, idx, torch.zeros_like(x)), gx)
    y, dout, (ga, gb) = _grad(lambda a, b: -0.5 * a + b, src, _randn(g, 6, 11))
    _close(R.axpy(torch.zeros_like(src), dout, -0.5), ga)
    assert torch.equal(R.axpy(dst, dst, 1.0), 2 * dst)


@pytest.mark.parametrize("op", ["prod", "lse"])
def test_reduce(op):
    g = _g(6)
    x = _randn(g, 3, 6, 4)
    if op == "prod":
        x = x.sign() * (x.abs() + 0.3)
    fwd = (lambda t: torch.prod(t, 1)) if op == "prod" else (lambda t: torch.logsumexp(t, 1))
    y, dout, (gx,) = _grad(fwd, x)
    _close(R.reduce_bwd(op, x, y, dout), gx)


def test_reduce_special_points():
    t = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    x = t([[[2.0], [0.0], [3.0], [-1.0]], [[2.0], [0.0], [0.0], [5.0]], [[2.0], [3.0], [4.0], [5.0]]])  # one zero, two zeros, dy == 0
    dy = t([[2.0], [7.0], [0.0]])
    got = R.reduce_bwd("prod", x, torch.prod(x, 1), dy)[..., 0]
    assert got.tolist() == [[0.0, -12.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]]
    xs = x.clone().requires_grad_(True)
    (torch.prod(xs, 1) * dy).sum().backward()
    assert torch.equal(xs.grad[..., 0], got)  # (torch takes the product of the others there as well)
    x = t([[[-INF], [0.5], [-INF]], [[-INF], [-INF], [-INF]], [[0.1], [0.2], [0.3]]])  # some -inf, all -inf, dy == 0
    dy = t([[2.0], [3.0], [0.0]])
    got = R.reduce_bwd("lse", x, torch.logsumexp(x, 1), dy)[..., 0]
    assert got.tolist() == [[0.0, 2.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]


@pytest.mark.parametrize("n1,n2", [(1, 3), (4, 3), (2, 5)])
def test_outer_sum(n1, n2):
    g = _g(7)
    a, b = _randn(g, 3, n1, 2), _randn(g, 3, n2, 2)
    y, dout, (ga, gb) = _grad(lambda p, q: (p.unsqueeze(2) + q.unsqueeze(1)).reshape(3, n1 * n2, 2), a, b)
    _close(R.outer_sum_bwd(dout, n1, n2, 0), ga)
    _close(R.outer_sum_bwd(dout, n1, n2, 1), gb)


@pytest.mark.parametrize("Fo,K1,K2", [(1, 1, 1), (3, 4, 3), (2, 1, 33)])
def test_gaussian_products(Fo, K1, K2):
    g = _g(8)
    m1, m2 = _randn(g, Fo, K1) * 3, _randn(g, Fo, K2) * 3
    s1, s2 = _randn(g, Fo, K1).abs() + 0.3, _randn(g, Fo, K2).abs() + 0.3
    sh = [(K1,), (K1,), (K2,), (K2,)]
    mean = _node_graph("gaussian_product_mean", {}, sh, (K1 * K2,), Fo)
    _, dout, want = _grad(lambda a, b, c, d: eval_param(mean, {"t0": a, "t1": b, "t2": c, "t3": d}), m1, s1, m2, s2)
    for got, w in zip(R.gaussian_product_mean_bwd(m1, s1, m2, s2, dout), want):
        _close(got, w)
    logz = _node_graph("gaussian_product_log_partition", {}, sh, (K1 * K2,), Fo)
    _, dout, want = _grad(lambda a, b, c, d: eval_param(logz, {"t0": a, "t1": b, "t2": c, "t3": d}), m1, s1, m2, s2)
    for got, w in zip(R.gaussian_product_logz_bwd(m1, s1, m2, s2, dout), want):
        _close(got, w)
    std = _node_graph("gaussian_product_stddev", {}, [(K1,), (K2,)], (K1 * K2,), Fo)
    _, dout, want = _grad(lambda a, b: eval_param(std, {"t0": a, "t1": b}), s1, s2)
    for got, w in zip(R.gaussian_product_stddev_bwd(s1, s2, dout), want):
        _close(got, w)


def test_log_table():
    g = _g(9)
    Fo, K, C = 2, 5, 11
    theta = _randn(g, Fo, K, C)

    def fwd(t):
        return torch.cat([torch.log_softmax(t, -1).transpose(1, 2), torch.zeros(Fo, 1, K, dtype=t.dtype)], dim=1)

    table, dout, (gx,) = _grad(fwd, theta)
    _close(R.log_table_bwd(table, dout), gx)
    poisoned = dout.clone()
    poisoned[:, C] = float("nan")  # row C is ignored
    prior = _randn(g, Fo, K, C)
    _close(R.log_table_bwd(table, poisoned, prior), gx + prior)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_optimizer_five_steps(kind):
    g = _g(10)
    theta0 = _randn(g, 6, 32)
    grads = [_randn(g, 6, 32) * s for s in (1.0, 1e3, 1e-3, 1.0, 10.0)]
    p = torch.nn.Parameter(theta0.clone())
    lr, betas, eps = 0.05, (0.9, 0.999), 1e-8
    opt = torch.optim.SGD([p], lr=lr) if kind == "sgd" else torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    theta, m1, m2 = theta0.clone(), torch.zeros_like(theta0), torch.zeros_like(theta0)
    for step, gr in enumerate(grads, start=1):
        p.grad = gr.clone()
        opt.step()
        theta, m1, m2 = R.opt_step(kind, theta, gr, m1, m2, step, lr, betas, eps)
        _close(theta, p.detach())
        if kind == "adam":
            st = opt.state[p]
            _close(m1, st["exp_avg"])
            _close(m2, st["exp_avg_sq"])
        _close(R.updated_row_softmax(theta), torch.softmax(p.detach(), -1))
    assert torch.equal(R.opt_step("adam", theta0, torch.zeros_like(theta0), m1 * 0, m2 * 0, 1, lr)[0], theta0)  # (g = 0 from rest: no move)


def test_fp32_runs_stay_finite_and_typed():
    """Every function computes in the dtype it is given (the yardstick is the fp32 run)."""
    g = _g(11)
    w = torch.softmax(torch.randn(4, 9, generator=g), -1)
    assert R.softmax_bwd_rows(w, torch.randn(4, 9, generator=g), torch.randn(4, 9, generator=g)).dtype == torch.float32
    x = torch.randn(2, 3, 4, generator=g)
    assert R.reduce_bwd("lse", x, torch.logsumexp(x, 1), torch.randn(2, 4, generator=g)).dtype == torch.float32
    th, a, b = R.opt_step("adam", x, x, torch.zeros_like(x), torch.zeros_like(x), 3, 0.01)
    assert th.dtype == a.dtype == b.dtype == torch.float32 and bool(torch.isfinite(th).all())
