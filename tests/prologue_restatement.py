"""Plain restatement of what the parameter prologue writes (cirkit_amd/csrc/ck_param.hip: `ck_param_softmax_batch` kinds
0, 1, 2, 4, 5 and the per-node kernels `ck_param_softmax`, `ck_param_transpose_last2`, `ck_param_table_integral_row`,
`ck_param_binomial_table`), entry by entry, in torch on the host.

Every function computes in the dtype of its input: float64 gives the reference the GPU is compared with, float32 the
yardstick of tests/test_gpu_param_prologue.py ("the same computation done in fp32 by torch on the CPU").  Nothing here
shares code or index arithmetic with the kernels: the formulas are the ones of include/cirkit_hip.h and of the reference
layers they stand for (layers/input.py:399-421, 530-541; nodes.py:764-783)."""
from __future__ import annotations

import numpy as np
import torch


def softmax_rows(x: torch.Tensor, log_space: bool = False, dim: int = -1) -> torch.Tensor:
    """Kind 0 / `ck_param_softmax`: softmax (or log-softmax) along one axis."""
    return torch.log_softmax(x, dim=dim) if log_space else torch.softmax(x, dim=dim)


def tiled_positions() -> np.ndarray:
    """CK_W_TILED_F32 of one (32 outputs, 32 inputs) fold as documented in cirkit_hip.h / ck_tile.h: "dword (q, lane, t) =
    W[lane & 31][8 q + 4 (lane >> 5) + t]" with q in 0..3, lane in 0..63, t in 0..3 and the dwords stored in that order.
    Returns (1024, 2): the (output, input) pair held by every dword."""
    pos = np.zeros((1024, 2), dtype=np.int64)
    for q in range(4):
        for lane in range(64):
            for t in range(4):
                pos[(q * 64 + lane) * 4 + t] = (lane % 32, 8 * q + 4 * (lane // 32) + t)
    return pos


def to_tiled(w: torch.Tensor) -> torch.Tensor:
    """(F, 32, 32) row-major weights -> (F, 1024) in CK_W_TILED_F32 order (kind 2 writes softmax_rows in this order)."""
    pos = tiled_positions()
    return w[:, pos[:, 0], pos[:, 1]]


def log_table(theta: torch.Tensor) -> torch.Tensor:
    """Kind 1: (F, K, C) logits -> (F, C + 1, K) = log softmax over C, transposed; row C (the integral row) exactly 0."""
    F, K, C = theta.shape
    out = torch.zeros((F, C + 1, K), dtype=theta.dtype)
    out[:, :C] = torch.log_softmax(theta, dim=2).transpose(1, 2)
    return out


def table_dense(theta: torch.Tensor, dense_theta: torch.Tensor, idx=None) -> torch.Tensor:
    """Kinds 4 and 5: v[d, c, o] = log sum_k softmax(dense_theta[d])[o, k] exp(T[idx[d], c, k]), T = log_table(theta), row C
    included (T = 0 there, so v = log sum_k W = 0 up to rounding).  Kind 4 writes v; kind 5 writes (out, out2) with
    log(out) + out2[..., None] = v."""
    T = log_table(theta)
    if idx is not None:
        T = T[torch.as_tensor(idx, dtype=torch.long)]
    logw = torch.log_softmax(dense_theta, dim=2)  # (Fd, O, K)
    return torch.logsumexp(T[:, :, None, :] + logw[:, None, :, :], dim=3)  # (Fd, C + 1, O)


def binomial_table(p: torch.Tensor, is_logits: bool, total_count: int) -> torch.Tensor:
    """`ck_param_binomial_table`: (F, K) probabilities or logits -> (F, total_count + 2, K), row c the log-pmf of the value c
    (torch.distributions.Binomial.log_prob, what TorchBinomialLayer evaluates), the last row the integral row, 0."""
    F, K = p.shape
    n = torch.tensor(float(total_count), dtype=p.dtype)
    if not is_logits:
        # probs_to_logits of torch.distributions: the probability clamped to [eps, 1 - eps] first, eps that of the PARAMETER's
        # dtype -- fp32 in the reference and on the device, whatever precision this restatement then computes in
        eps = torch.finfo(torch.float32).eps
        q = p.clamp(min=eps, max=1.0 - eps)
        p = torch.log(q) - torch.log1p(-q)
    dist = torch.distributions.Binomial(n, logits=p[:, None, :])
    values = torch.arange(total_count + 1, dtype=p.dtype)[None, :, None].expand(F, total_count + 1, K)
    out = torch.zeros((F, total_count + 2, K), dtype=p.dtype)
    out[:, : total_count + 1] = dist.log_prob(values)
    return out


def integral_row(table: torch.Tensor, mode: int) -> torch.Tensor:
    """`ck_param_table_integral_row` on a (F, C + 1, K) table: the values of row C.  Mode 0: zeros (normalised
    probabilities); 1: logsumexp over the C rows (unnormalised logits, input.py:414-421); 2: ones (embedding tables);
    3: complex ones, K floats = K / 2 pairs (1, 0)."""
    F, C1, K = table.shape
    if mode == 0:
        return torch.zeros((F, K), dtype=table.dtype)
    if mode == 1:
        return torch.logsumexp(table[:, : C1 - 1], dim=1)
    if mode == 2:
        return torch.ones((F, K), dtype=table.dtype)
    if mode == 3:
        row = torch.zeros((F, K), dtype=table.dtype)
        row[:, 0::2] = 1
        return row
    raise ValueError(mode)


def transpose_last2(x: torch.Tensor, take_log: bool = False) -> torch.Tensor:
    """`ck_param_transpose_last2`: (R, A, Bd) -> (R, Bd, A), optionally the log of every entry (log 0 = -inf).  With
    out_rows > Bd the kernel writes these Bd rows of every (out_rows, A) block and leaves the others alone."""
    y = x.transpose(1, 2).contiguous()
    return torch.log(y) if take_log else y
