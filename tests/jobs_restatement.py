"""Plain restatement of the job-form training step, one function per contract of include/cirkit_hip.h, "training step as job lists"
(cirkit_amd/csrc/ck_jobs.hip: `ck_jobs_sum64_fwd` / `_bwd`, `ck_jobs_mix_fwd` / `_bwd`, `ck_jobs_mix_params`, `ck_jobs_nsum`,
`ck_jobs_root`, `ck_jobs_cat_bwd`, `ck_jobs_gauss_bwd`), in torch on the host.  Blocks are (rows, 64) tensors; a job's rows are all
the rows given (the caller slices [row0, row1) itself: a job cut into units computes what the uncut job computes).

Every function computes in the dtype of its inputs: float64 gives the reference the GPU is compared with, float32 the yardstick of
tests/test_gpu_jobs.py.  None goes through autograd; tests/test_jobs_restatement.py pins them to torch autograd in fp64.
The sum job's backward IS `layer_backward_restatement.sum_lse_grads` on one fold with one child; its forward and the mixing fold
under it need y and the row maximum, which that module does not return, so `_sum_terms` forms them.  The mixing job does not go
through `mixing_lse_terms`: that shifts by the maximum of the whole ROW, the kernels by the maximum PER UNIT (the value is the
same; in fp32 the row's maximum lets a unit 87 nats below it underflow, and the yardstick of a spread case would not be finite).

Mode 0 returns the gradient of the linear weights, mode 1 the gradient of the logits behind their softmax.  Mode 2 has no function
of its own: it is `opt_step` (param_backward_restatement's, on the device state's clock) on the mode-1 gradient, then
`updated_row_softmax` (sum, mixing, root), `prologue_restatement.log_table` (Categorical) or the scaled sigmoid (Gaussian) of the updated tensor.

Conventions that differ from what autograd gives, on purpose (the contract of the header):
* where y = 0 (a row whose inputs are all -inf, or that meets only zero weights) or G = 0 the term G / y is 0: such a row has
  gradient 0 and adds nothing to the parameters' gradients (autograd: NaN);
* a category x < 0 (marginalised) selects row C of a Categorical table, x >= C row C - 1;
* a NaN x of a Gaussian fold contributes nothing;
* `mix_dw[:, h]` = s / w is 0 where the coefficient w is exactly 0."""
from __future__ import annotations

import torch

from layer_backward_restatement import PROD, _clamped_max, _guarded_ratio, gaussian_terms, sum_lse_grads, sum_lse_terms
from param_backward_restatement import log_table_bwd, opt_step as P_opt_step, scaled_sigmoid_bwd, softmax_bwd_rows


def opt_step(kind, theta, g, m1, m2, step, lr, betas32, betas, eps):
    """`param_backward_restatement.opt_step` with the clock of the DEVICE `ck_opt_state` (include/cirkit_hip.h): the moments are
    updated with the fp32 betas the state holds (`betas32`, b m + (1 - b) g), the bias corrections are 1 - b^step of the DOUBLE
    betas (`ck_opt_tick` forms them in double from b1d / b2d, as torch.optim.Adam does)."""
    th, m1n, m2n = P_opt_step(kind, theta, g, m1, m2, step, lr, betas32, eps)
    if kind == "sgd":
        return th, m1n, m2n
    bc1, bc2 = 1.0 - float(betas[0]) ** int(step), 1.0 - float(betas[1]) ** int(step)
    return theta - (lr / bc1) * m1n / (torch.sqrt(m2n) / bc2 ** 0.5 + eps), m1n, m2n


def nsum(blocks):
    """`ck_jobs_nsum`: the blocks added in list order, starting from the first one (in fp32: one rounding per addition, so the
    fp32 run is what the kernel must return bit for bit)."""
    a = blocks[0].clone()
    for b in blocks[1:]:
        a = a + b
    return a


def input_rows(xrow, C):
    """The table row every batch row selects: x < 0 -> C, x >= C -> C - 1."""
    x = xrow.long()
    return torch.where(x < 0, torch.full_like(x, C), x.clamp(max=C - 1))


def _sum_terms(blocks, W, xrow, table):
    """(e (B, 64), y (B, 64), m (B, 1)) of out = log(W e) + m: v = the sum of the blocks, or the rows of `table` (C + 1, 64) that
    `xrow` selects; m the clamped maximum of the row."""
    v = nsum(blocks) if xrow is None else table[input_rows(xrow, table.shape[0] - 1)]
    m = _clamped_max(v, -1)
    e = torch.exp(v - m)
    return e, e @ W.t(), m


def sum_job_fwd(blocks, W, xrow=None, table=None):
    """`ck_jobs_sum64_fwd`: out (B, 64) = log(W exp(v - m)) + m.  A row of -inf gives -inf."""
    e, y, m = _sum_terms(blocks, W, xrow, table)
    return torch.log(y) + m


def sum_job_bwd(blocks, W, glist, mode, xrow=None, table=None, mix_out=None, mix_w=None, mix_h=0, partners=()):
    """`ck_jobs_sum64_bwd`: (gx (B, 64), dtheta (64, 64), mix_dw column (64) or None).  G = the sum of the gradient list; with
    `mix_out` (B, 64), the output of the mixing fold above, taken as given: G = (the sum) w[:, h] exp(x_h - mix_out) with x_h = this
    job's output plus the `partners` blocks and w = mix_w (64, H).  gx = e W^T (G / y), dW = (G / y)^T e; mode 0: dW; mode 1:
    W (dW - <W, dW>).  mix_dw[:, h] = <W, dW> / w = sum_b G / w, 0 where w = 0."""
    e, y, m = _sum_terms(blocks, W, xrow, table)
    G = nsum(glist)
    s_over_w = None
    if mix_out is not None:
        xh = torch.log(y) + m
        for p in partners:
            xh = xh + p
        w = mix_w[:, mix_h]
        live = (y > 0) & (G != 0) & (w > 0)
        d = torch.where(live, xh - mix_out, torch.zeros_like(xh))
        G = torch.where(live, G * w * torch.exp(d), torch.zeros_like(G))
    # the layer itself is `ck_sum_lse_bwd` on ONE fold with ONE child, v: its restatement does the rest
    v = nsum(blocks) if xrow is None else table[input_rows(xrow, table.shape[0] - 1)]
    args = (v.reshape(-1), [[0]], W.unsqueeze(0), G.unsqueeze(0), v.shape[0], v.shape[1], PROD)
    gx, dW = sum_lse_grads(*args, sum_lse_terms(*args))
    gx, dW = gx[0, 0], dW[0]
    if mix_out is not None:
        s = (W * dW).sum(-1)
        s_over_w = torch.where(w > 0, s / torch.where(w > 0, w, torch.ones_like(w)), torch.zeros_like(s))
    return gx, (dW if mode == 0 else softmax_bwd_rows(W, dW)), s_over_w


def _mix_terms(slots, w):
    """(e (H, B, 64), y (B, 64), m (B, 64)): slot h = the sum of its blocks in list order, m the clamped maximum PER UNIT over the
    slots (the value is the same for any shift that bounds the unit's own inputs), e_h = exp(x_h - m), y = sum_h w[:, h] e_h."""
    x = torch.stack([nsum(s) for s in slots])
    m = _clamped_max(x, 0)
    e = torch.exp(x - m)
    return e, (e * w.t().unsqueeze(1)).sum(0), m[0]


def mix_job_fwd(slots, w):
    """`ck_jobs_mix_fwd`: slots = H lists of S blocks (B, 64), w (64, H); out[k] = log(sum_h w[k, h] e_h[k]) + m[k]."""
    e, y, m = _mix_terms(slots, w)
    return torch.log(y) + m


def mix_params(dw, w, mode):
    """`ck_jobs_mix_params`: the parameter step of a mixing fold from d w (64, H): mode 0 d w itself, mode 1 w (dw - <w, dw>),
    the softmax running over h."""
    return dw if mode == 0 else softmax_bwd_rows(w, dw)


def mix_job_bwd(slots, w, glist, mode):
    """`ck_jobs_mix_bwd`: (gx (H, B, 64), dtheta (64, H)).  gx_h[k] = G[k] w[k, h] e_h[k] / y[k], d w[k, h] = sum_b G[k] e_h[k] / y[k]."""
    e, y, m = _mix_terms(slots, w)
    ge = _guarded_ratio(nsum(glist), y).unsqueeze(0) * e
    return ge * w.t().unsqueeze(1), mix_params(ge.sum(1).t(), w, mode)


def root(folds, W, c, mode, seed=None, seed_const=0.0, bad=False):
    """`ck_jobs_root`: folds = R lists of S blocks (B, 64), W (R, 64), c (R) or None (R = 1).  o_r = log(sum_n W[r, n] exp(v_r[n] -
    m_r)) + m_r, out = log(sum_r c_r exp(o_r - M)) + M (c None: o_0).  Returns (out (B), ll = [sum out, B], gx (R, B, 64),
    dtheta_w (R, 64), dtheta_c (R) or None) for loss = sum_b seed_b out_b (`seed` (B), or `seed_const` for every row).  `bad`:
    every out is NaN (the gradients are those of the values)."""
    v = torch.stack([nsum(f) for f in folds])  # (R, B, 64)
    R, B = v.shape[:2]
    m = _clamped_max(v, -1)
    e = torch.exp(v - m)
    y = (e * W.unsqueeze(1)).sum(-1, keepdim=True)  # (R, B, 1)
    o = (torch.log(y) + m).squeeze(-1)  # (R, B)
    if c is None:
        out, p, Y, cr = o[0].clone(), torch.ones_like(o), torch.ones_like(o[0]), torch.ones(1, dtype=v.dtype)
    else:
        M = _clamped_max(o, 0)
        p = torch.exp(o - M)
        Y = (c.unsqueeze(1) * p).sum(0)
        out, cr = torch.log(Y) + M[0], c
    sd = torch.full((B,), seed_const, dtype=v.dtype) if seed is None else seed
    q = torch.where(Y > 0, sd * p / torch.where(Y > 0, Y, torch.ones_like(Y)), torch.zeros_like(p))  # (R, B)
    t = torch.where(y > 0, (q * cr.unsqueeze(1)).unsqueeze(-1) * e / torch.where(y > 0, y, torch.ones_like(y)), torch.zeros_like(e))
    gx = t * W.unsqueeze(1)
    dw, dc = t.sum(1), q.sum(1)
    if mode != 0:
        dw = softmax_bwd_rows(W, dw)
        dc = softmax_bwd_rows(c.unsqueeze(0), dc.unsqueeze(0))[0] if c is not None else None
    if bad:
        out = torch.full_like(out, float("nan"))
    return out, torch.stack([out.sum(), torch.tensor(float(B), dtype=v.dtype)]), gx, dw, (dc if c is not None else None)


def cat_histogram(G, x, C):
    """(C + 1, 64): the scatter-add of the rows of G (B, 64) by the table row their category selects."""
    return torch.zeros(C + 1, G.shape[1], dtype=G.dtype).index_add_(0, input_rows(x, C), G)


def cat_job_bwd(G, x, theta, table=None):
    """`ck_jobs_cat_bwd`, mode 1: d theta (64, C) for out[b, :] = log softmax(theta)[:, x_b]: the scatter of G by category, the
    marginalised row C dropped, through the log-softmax: d theta[k, c] = dT[c, k] - p[k, c] sum_c' dT[c', k].  `table` (C + 1, 64),
    what the forward gathered from, holds log p transposed; None: it is formed from theta in theta's dtype (the reference and the
    yardstick do that, so that neither inherits the rounding of an fp32 table)."""
    C = theta.shape[1]
    if table is None:
        table = torch.zeros(C + 1, theta.shape[0], dtype=theta.dtype)
        table[:C] = torch.log_softmax(theta, -1).t()
    return log_table_bwd(table.unsqueeze(0), cat_histogram(G, x, C).unsqueeze(0))[0]


def gauss_job_bwd(G, x, mean, stddev, vmin=0.0, vmax=1.0, has_ss=False):
    """`ck_jobs_gauss_bwd`, mode 1: (dmean (64), dsd (64)) for log N(x_b; mean, stddev); has_ss: dsd is the gradient of the tensor
    behind stddev = vmin + (vmax - vmin) sigmoid(theta).  A NaN x contributes nothing."""
    tm, ts = gaussian_terms(G.unsqueeze(0), x.unsqueeze(0), [0], mean.unsqueeze(0), stddev.unsqueeze(0))
    dm, ds = tm.sum(1)[0], ts.sum(1)[0]
    return dm, (scaled_sigmoid_bwd(stddev, ds, vmin, vmax) if has_ss else ds)
