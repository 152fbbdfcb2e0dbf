#!/usr/bin/env python3
"""Pairwise mutual information for Chow-Liu structure learning (`cirkit_amd.structure.pairwise_mutual_information`,
DESIGN.md section 11 "Structure learning") on synthetic MNIST-shaped data: N = 60000 rows, D = 784 features, 256 states --
as they are, in 32 bins and in 8 bins; following scripts/bench_classifier.py's protocol.

    python scripts/bench_chow_liu.py [--reps 3] [--warmup 1] [--rows 60000] [--features 784] [--torch-chunk 256]

HIP events around each timed call after `--warmup` untimed ones; the median is reported.  A timed call is the whole public
function: staging, marginals and the pair kernel.  "Effective one-hot FLOP/s" counts the upper triangle of the Gram matrix
of the one-hot encoding over the C real states, 2 N (D C)^2 / 2 operations per call, whatever the kernel pads.  At 8 bins
the reference's formulation (a (D, D, C^2) int64 count tensor filled by scatter_add_, chow_liu.py:107-151) is timed in
torch on the same device, in chunks of `--torch-chunk` rows (a chunk's index tensor is D^2 x chunk int64), and the two
matrices are compared.  Prints one JSON line.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cirkit_amd.structure import pairwise_mutual_information  # noqa: E402


def _time(fn, reps: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def torch_formulation(x: torch.Tensor, c: int, chunk: int, alpha: float = 0.01) -> torch.Tensor:
    """The reference's `_categorical_mutual_info` written out in torch (fp32 like the reference) on the device of `x`."""
    n, d = x.shape
    counts = torch.zeros(d, d, c * c, dtype=torch.long, device=x.device)
    for part in x.split(chunk):
        pair = part.t().unsqueeze(1) * c + part.t().unsqueeze(0)
        counts.scatter_add_(-1, pair, torch.ones_like(pair))
    counts = counts.view(d, d, c, c)
    feat, cats = torch.arange(d, device=x.device), torch.arange(c, device=x.device)
    denom = n + c * c * alpha
    marg = (counts[feat, feat][:, cats, cats] + c * alpha) / denom
    joint = (counts + alpha) / denom
    joint[feat, feat] = torch.diag_embed(marg)
    indep = torch.einsum("ik,jl->ijkl", marg, marg)
    return (joint * (joint.log() - indep.log())).sum(dim=(2, 3)).fill_diagonal_(0)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--features", type=int, default=784)
    ap.add_argument("--torch-chunk", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, d = args.rows, args.features
    g = torch.Generator().manual_seed(4)
    # neighbouring pixels agree on most rows, so the matrix has a structure to find
    x = torch.randint(0, 256, (n, d), generator=g)
    copy = torch.rand((n, d), generator=g) < 0.6
    for j in range(1, d):
        x[:, j] = torch.where(copy[:, j], x[:, j - 1], x[:, j])
    x = x.to(dev)
    row = {"N": n, "D": d}
    for bins in (None, 32, 8):
        c = 256 if bins is None else bins
        ms = _time(lambda: pairwise_mutual_information(x, 256, num_bins=bins), args.reps, args.warmup)
        row[f"C{c}"] = {"ms": round(ms, 2), "rows_per_s": round(n / ms * 1e3), "onehot_TFLOPs": round(n * float(d * c) ** 2 / ms / 1e9, 2)}
    xb = torch.div(x, 32, rounding_mode="floor")
    kept = []
    ms = _time(lambda: kept.append(torch_formulation(xb, 8, args.torch_chunk)), 1, 1)
    ours = pairwise_mutual_information(x, 256, num_bins=8)
    diff = float((kept[-1].double() - ours).abs().max())
    row["torch_C8"] = {"ms": round(ms, 2), "rows_per_s": round(n / ms * 1e3), "chunk": args.torch_chunk, "max_abs_diff_fp32_vs_ours": diff}
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
