"""Plain restatement of the reverse half of the parameter graphs, one function per kernel (cirkit_amd/csrc/ck_backward.hip,
ck_param.hip: the launches `HipParameter.backward` and the trainers drive), entry by entry, in torch on the host.

Every function computes in the dtype of its inputs: float64 gives the reference the GPU is compared with, float32 the
yardstick of tests/test_gpu_param_backward.py.  None goes through autograd: the formulas are the ones written above the kernels
and the derivatives of the reference's node forwards (parameters/nodes.py); tests/test_param_backward_restatement.py pins them to
torch autograd in fp64.  Where a kernel adds into its output, the function takes `accumulate`: None (the gradient is written) or
the prior value of the output, which is added in the function's own dtype.

Conventions that differ from what autograd gives, on purpose:
* `unary_bwd`: an entry with dy == 0 has gradient exactly 0 whatever the derivative (log at x == 0: autograd gives 0 * inf = NaN);
  the same rule holds in `reduce_bwd`.
* `unary_bwd` "clamp": the derivative is 1 on [vmin, vmax], both bounds INCLUDED (torch.clamp's backward), 0 outside.
* `unary_bwd` "softplus": torch's threshold of 20 -- above it the forward is the identity and the derivative 1.
* `reduce_bwd` "prod": an entry equal to 0 takes the product of the OTHER entries of its line (dy y / x elsewhere).
* `reduce_bwd` "lse": a line that is all -inf (y = -inf) has gradient 0 (autograd: NaN); one whose y is +inf too."""
from __future__ import annotations

import torch


def _out(g: torch.Tensor, accumulate: torch.Tensor | None) -> torch.Tensor:
    return g if accumulate is None else accumulate.to(g.dtype) + g


def softmax_bwd_rows(w, dw, accumulate=None):
    """`ck_param_softmax_bwd`: w (rows, len) = softmax(theta) over the last axis; dtheta = w (dw - sum_l w dw)."""
    return _out(w * (dw - (w * dw).sum(dim=-1, keepdim=True)), accumulate)


def softmax_bwd_strided(y, dy, log_space, accumulate=None):
    """`ck_param_softmax_bwd_strided`: y (outer, len, inner) the node's OUTPUT along axis 1.
    softmax: dx = y (dy - sum_l y dy); log-softmax: dx = dy - exp(y) sum_l dy (so dx = dy where y = -inf)."""
    if log_space:
        return _out(dy - torch.exp(y) * dy.sum(dim=1, keepdim=True), accumulate)
    return _out(y * (dy - (y * dy).sum(dim=1, keepdim=True)), accumulate)


UNARY_OPS = ("sigmoid", "exp", "log", "square", "clamp", "softplus")


def unary_bwd(op, x, y, dy, accumulate=None, vmin=None, vmax=None):
    """`ck_param_unary_bwd` from the node's input x and output y: sigmoid y (1 - y); exp y; log 1 / x; square 2 x; clamp 1 on
    [vmin, vmax] (bounds included, an absent bound is open) else 0; softplus 1 / (1 + exp(-x)), and 1 above x = 20.
    dy == 0 gives exactly 0 (also at log(0), where the derivative is inf)."""
    if op == "sigmoid":
        d = y * (1 - y)
    elif op == "exp":
        d = y
    elif op == "log":
        d = 1 / x
    elif op == "square":
        d = 2 * x
    elif op == "clamp":
        inside = torch.ones_like(x, dtype=torch.bool)
        if vmin is not None:
            inside &= x >= vmin
        if vmax is not None:
            inside &= x <= vmax
        d = inside.to(x.dtype)
    elif op == "softplus":
        d = torch.where(x > 20, torch.ones_like(x), 1 / (1 + torch.exp(-x)))
    else:
        raise ValueError(op)
    return _out(torch.where(dy == 0, torch.zeros_like(dy), dy * d), accumulate)


def scaled_sigmoid_bwd(y, dy, vmin, vmax, accumulate=None):
    """`ck_param_scaled_sigmoid_bwd`: y = sigmoid(x) (vmax - vmin) + vmin, dx = dy (y - vmin) (vmax - y) / (vmax - vmin)."""
    return _out(dy * (y - vmin) * (vmax - y) / (vmax - vmin), accumulate)


def mixing_weight_bwd(dy, K, H, accumulate=None):
    """`ck_param_mixing_weight_bwd`: the forward lays x (F, K, H) out block-diagonally, y[f, k, h K + k] = x[f, k, h]; the
    backward picks those entries: dx[f, k, h] = dy[f, k, h K + k].  Nothing else of dy is read."""
    F = dy.shape[0]
    picks = torch.diagonal(dy.reshape(F, K, H, K), dim1=1, dim2=3)  # (F, H, K): entry [f, h, k] = dy[f, k, h, k]
    return _out(picks.permute(0, 2, 1).contiguous(), accumulate)


def scatter_add_folds(dsrc, idx, ddst):
    """`ck_param_scatter_add_folds`: ddst[idx[i]] += dsrc[i] for every row i, duplicates in idx included."""
    out = ddst.clone()
    for i, d in enumerate(idx.tolist()):
        out[d] = out[d] + dsrc[i]
    return out


def axpy(y, x, a):
    """`ck_axpy_f32`: a x + y."""
    return a * x + y


def reduce_bwd(op, x, y, dy):
    """`ck_param_reduce_bwd`: x (outer, len, inner) reduced along axis 1 to y (outer, inner), dy likewise.
    "prod": dx = dy y / x, and dy times the product of the other entries of the line where x == 0.
    "lse":  dx = dy exp(x - y); 0 on a line whose y is not finite (all -inf).   dy == 0 gives exactly 0 on its line."""
    ln = x.shape[1]
    if op == "prod":
        others = torch.ones_like(x)
        for j in range(ln):
            for k in range(ln):
                if k != j:
                    others[:, j] = others[:, j] * x[:, k]
        d = torch.where(x != 0, y.unsqueeze(1) / torch.where(x != 0, x, torch.ones_like(x)), others)
    elif op == "lse":
        yy = y.unsqueeze(1).expand_as(x)
        live = torch.isfinite(yy)
        d = torch.where(live, torch.exp(torch.where(live, x - yy, torch.zeros_like(x))), torch.zeros_like(x))
    else:
        raise ValueError(op)
    g = dy.unsqueeze(1).expand_as(x)
    return torch.where(g == 0, torch.zeros_like(x), g * d)


def outer_sum_bwd(dout, n1, n2, which):
    """`ck_param_outer_sum_bwd`: out[o, i1 n2 + i2, r] = a[o, i1, r] + b[o, i2, r]; da = sum over i2 (which 0), db = sum
    over i1 (which 1) of dout (outer, n1 n2, inner)."""
    d = dout.reshape(dout.shape[0], n1, n2, dout.shape[-1])
    return d.sum(dim=2) if which == 0 else d.sum(dim=1)


def gaussian_product_mean_bwd(m1, s1, m2, s2, dout):
    """`ck_param_gaussian_product_ms_bwd`, op 0.  mean[f, i, j] = (m1_i v2_j + m2_j v1_i) / D, v = s^2, D = v1_i + v2_j:
    d/dm1 = v2 / D, d/dm2 = v1 / D, d/ds1 = 2 s1 (m2 - mean) / D, d/ds2 = 2 s2 (m1 - mean) / D, each times dout (F, K1 K2) and
    summed over the other operand's units.  Returns (dm1, ds1, dm2, ds2)."""
    g = dout.reshape(m1.shape[0], m1.shape[1], m2.shape[1])
    v1, v2 = (s1 * s1).unsqueeze(2), (s2 * s2).unsqueeze(1)
    D = v1 + v2
    mean = (m1.unsqueeze(2) * v2 + m2.unsqueeze(1) * v1) / D
    dm1, dm2 = (g * v2 / D).sum(2), (g * v1 / D).sum(1)
    ds1 = (g * 2 * s1.unsqueeze(2) * (m2.unsqueeze(1) - mean) / D).sum(2)
    ds2 = (g * 2 * s2.unsqueeze(1) * (m1.unsqueeze(2) - mean) / D).sum(1)
    return dm1, ds1, dm2, ds2


def gaussian_product_stddev_bwd(s1, s2, dout):
    """`ck_param_gaussian_product_ms_bwd`, op 1.  out = sqrt(v1 v2 / D): d/ds1 = (s1 / out) v2^2 / D^2, d/ds2 = (s2 / out)
    v1^2 / D^2.  Returns (ds1, ds2)."""
    g = dout.reshape(s1.shape[0], s1.shape[1], s2.shape[1])
    v1, v2 = (s1 * s1).unsqueeze(2), (s2 * s2).unsqueeze(1)
    D = v1 + v2
    out = torch.sqrt(v1 * v2 / D)
    ds1 = (g * (s1.unsqueeze(2) / out) * v2 * v2 / (D * D)).sum(2)
    ds2 = (g * (s2.unsqueeze(1) / out) * v1 * v1 / (D * D)).sum(1)
    return ds1, ds2


def gaussian_product_logz_bwd(m1, s1, m2, s2, dout):
    """`ck_param_gaussian_product_logz_bwd`.  out[f, i, j] = -0.5 (log 2 pi + log v + d^2 / v), v = s1_i^2 + s2_j^2, d = m1_i - m2_j:
    d/dm1 = -d / v, d/dm2 = d / v, d/ds1 = s1 (d^2 / v - 1) / v, d/ds2 = s2 (d^2 / v - 1) / v.  Returns (dm1, ds1, dm2, ds2)."""
    g = dout.reshape(m1.shape[0], m1.shape[1], m2.shape[1])
    v = (s1 * s1).unsqueeze(2) + (s2 * s2).unsqueeze(1)
    d = m1.unsqueeze(2) - m2.unsqueeze(1)
    t = g * (d * d / v - 1) / v
    return (-(g * d / v)).sum(2), (t * s1.unsqueeze(2)).sum(2), (g * d / v).sum(1), (t * s2.unsqueeze(1)).sum(1)


def log_table_bwd(table, dtable, accumulate=None):
    """`ck_param_log_table_bwd`: table (F, C + 1, K) = log softmax over C of theta (F, K, C), transposed, row C the integral row;
    dtheta[f, k, c] = dT[f, c, k] - exp(T[f, c, k]) sum_c' dT[f, c', k] over the rows c' < C.  Row C of both is ignored."""
    C = table.shape[1] - 1
    T, dT = table[:, :C], dtable[:, :C]
    g = dT - torch.exp(T) * dT.sum(dim=1, keepdim=True)
    return _out(g.transpose(1, 2).contiguous(), accumulate)


def opt_step(kind, theta, g, m1, m2, step, lr, betas=(0.9, 0.999), eps=1e-8):
    """One optimizer step on an entry.  "sgd": theta - lr g.  "adam": torch.optim.Adam without weight decay or amsgrad at its
    step-th step (1-based): m1' = b1 m1 + (1 - b1) g, m2' = b2 m2 + (1 - b2) g^2, the bias corrections 1 - b^step formed in
    double, theta' = theta - (lr / bc1) m1' / (sqrt(m2') / sqrt(bc2) + eps).  Returns (theta', m1', m2')."""
    if kind == "sgd":
        return theta - lr * g, m1, m2
    b1, b2 = float(betas[0]), float(betas[1])
    bc1, bc2 = 1.0 - b1 ** int(step), 1.0 - b2 ** int(step)
    m1n = b1 * m1 + (1 - b1) * g
    m2n = b2 * m2 + (1 - b2) * g * g
    return theta - (lr / bc1) * m1n / (torch.sqrt(m2n) / bc2 ** 0.5 + eps), m1n, m2n


def updated_row_softmax(theta):
    """What the optimizer epilogue leaves for the next forward: the softmax of the updated logits over the last axis."""
    e = torch.exp(theta - theta.amax(dim=-1, keepdim=True))
    return e / e.sum(dim=-1, keepdim=True)
