#!/usr/bin/env python3
"""Autoregressive conditionals and coding (`HipCircuit.autoregressive_log_probs`, `HipCircuit.coding_tables`,
cirkit_amd/codec.py; DESIGN.md section 11 "Autoregressive conditionals and coding") at BASELINE config 2 (QuadTree-2,
Categorical-256, K = 32, 784 variables) at 1, 8 and 64 rows drawn from the circuit, following
scripts/bench_leave_one_out.py's protocol.

    python scripts/bench_autoregressive.py [--reps 20] [--warmup 5] [--batches 1,8,64] [--no-decode]

HIP events around each timed call after `--warmup` untimed ones; the median is reported.  Per batch size: the whole
`autoregressive_log_probs` call and the whole `coding_tables` call (all 784 steps, B x 784 expanded rows in chunks), then ONE
stepwise `compress` and ONE stepwise `decompress` by the wall clock (784 `coding_tables` calls of B rows each, with the table
copied to the host every step), the round trip checked, and the compressed bits per dimension next to the quantised ideal and
to -log2 p(x) / D from the log probabilities.  For comparison only: the composition a user could already write, the batch
expanded on the host and `leave_one_out` gathered on the diagonal -- on the 4 x 4 Categorical-256 image circuit at every batch
size and on config 2 at one row (above that its (B D, D, C) output does not fit).  Prints one JSON line per measurement.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cirkit_amd import codec  # noqa: E402
from cirkit_amd.circuit import HipCircuit  # noqa: E402
from cirkit_amd.initializers import init_plan_tensors  # noqa: E402
from cirkit_amd.leave_one_out import _loo  # noqa: E402
from cirkit_amd.plan import Plan  # noqa: E402
from cirkit_amd.templates import image_data  # noqa: E402


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


def _composition(hc: HipCircuit, x: torch.Tensor) -> torch.Tensor:
    """(B, D, C): the batch expanded on the host, `leave_one_out` on all of it, the diagonal gathered."""
    B, D = x.shape
    hide = torch.arange(D)[None, :] >= torch.arange(D)[:, None]  # (step, variable)
    xe = x.cpu().repeat_interleave(D, dim=0)
    mask = hide.repeat(B, 1)
    full = hc.leave_one_out(xe.to(hc.device), None, mask.to(hc.device))
    rows = torch.arange(B * D, device=hc.device)
    return full[rows, rows % D].reshape(B, D, -1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--no-decode", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    batches = [int(b) for b in args.batches.split(",")]
    plan = Plan.load(os.path.join(ROOT, "tests", "golden", "cfg2_qt784"))
    hc = HipCircuit(plan, init_plan_tensors(plan), device=dev)
    small_plan = image_data((1, 4, 4), region_graph="quad-tree-2", input_layer="categorical", num_input_units=32,
                            sum_product_layer="cp", num_sum_units=32)
    small = HipCircuit(small_plan, init_plan_tensors(small_plan, seed=5), device=dev)
    D = plan.num_variables
    for B in batches:
        x = hc.sample(B, seed=2)
        lp = hc.autoregressive_log_probs(x)
        chunks = _loo(hc).down.chunks_of(B * D, None)
        row = {"config": "config 2", "plan": "cfg2_qt784", "B": B, "D": D, "expanded_rows": B * D, "chunks": len(chunks),
               "rows_per_chunk": chunks[0][1],
               "autoregressive_log_probs_ms": round(_time(lambda: hc.autoregressive_log_probs(x), args.reps, args.warmup), 4),
               "coding_tables_ms": round(_time(lambda: hc.coding_tables(x), args.reps, args.warmup), 4),
               "one_step_coding_tables_ms": round(_time(lambda: hc.coding_tables(x, positions=[D // 2]), args.reps, args.warmup), 4),
               "minus_log2_p_per_dim": round(float(-lp.double().sum(1).mean()) / np.log(2) / D, 4)}
        if not args.no_decode:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            blobs, counts = codec.compress(hc, x, return_counts=True)
            t1 = time.perf_counter()
            back = codec.decompress(hc, blobs)
            t2 = time.perf_counter()
            assert torch.equal(back, x.cpu()), "round trip"
            batched = codec.compress(hc, x, batched=True)
            assert batched == blobs, "batched tables differ from the stepwise ones"
            bits = np.array([8 * len(b) for b in blobs])
            row.update(stepwise_compress_s=round(t1 - t0, 3), stepwise_decompress_s=round(t2 - t1, 3),
                       compressed_bits_per_dim=round(float(bits.mean()) / D, 4),
                       quantised_ideal_bits_per_dim=round(float(codec.ideal_bits(counts, 16).mean()) / D, 4))
        print(json.dumps(row), flush=True)
        xs = small.sample(B, seed=3)
        a = small.autoregressive_conditionals(xs)
        assert torch.equal(a, _composition(small, xs)), "the composition differs"
        print(json.dumps({"plan": "4x4 Categorical-256 K=32", "B": B, "D": 16,
                          "autoregressive_conditionals_ms": round(_time(lambda: small.autoregressive_conditionals(xs), args.reps, args.warmup), 4),
                          "host_expanded_leave_one_out_ms": round(_time(lambda: _composition(small, xs), args.reps, args.warmup), 4)}),
              flush=True)
        del lp
        torch.cuda.empty_cache()
    x = hc.sample(1, seed=2)
    a = hc.autoregressive_conditionals(x)
    assert torch.equal(a, _composition(hc, x)), "the composition differs"
    del a
    print(json.dumps({"config": "config 2", "plan": "cfg2_qt784", "B": 1, "D": D,
                      "autoregressive_conditionals_ms": round(_time(lambda: hc.autoregressive_conditionals(x), args.reps, args.warmup), 4),
                      "host_expanded_leave_one_out_ms": round(_time(lambda: _composition(hc, x), max(3, args.reps // 4), 2), 4)}),
          flush=True)


if __name__ == "__main__":
    main()
