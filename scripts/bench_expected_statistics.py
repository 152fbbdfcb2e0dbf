#!/usr/bin/env python3
"""Expected-statistics time (`HipCircuit.expected_statistics`, DESIGN.md section 11 "Expected statistics") at BASELINE config 2
(QuadTree-2, Categorical-256, K = 32; 4096 rows) and config 4 (Poon-Domingos, Gaussian, K = 64; 1024 rows), the lower half of
the variables missing, following scripts/bench_posterior.py's protocol.

    python scripts/bench_expected_statistics.py [--reps 20] [--warmup 5]

HIP events around each timed call after `--warmup` untimed ones; the median is reported.  Per config: the whole call, and its
phases replayed one by one on what the last call left -- the evidence forwards of every chunk (range check included), the
flow passes, and the three statistics phases (unit sums, edge contraction, leaf sums).  The yardstick is evidence forward +
flow pass, what `posterior_marginals` costs before its leaves; the statistics phases are reported as a multiple of it.  The
edge contraction is also reported against its floor, the larger of 2 rows Ko M FLOP per fold at the fp32 matrix-core rate
DESIGN.md section 4 measured (157.3 TFLOP/s) and one read of the value and flow arenas at the measured copy rate (6.0 TB/s).
Prints one JSON line per config.
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

from cirkit_amd.circuit import HipCircuit  # noqa: E402
from cirkit_amd.expected import _expected  # noqa: E402
from cirkit_amd.initializers import init_plan_tensors  # noqa: E402
from cirkit_amd.plan import Plan  # noqa: E402
from cirkit_amd.topdown import SUM_KINDS  # noqa: E402

CONFIGS = {"cfg2_qt784": ("config 2", 4096), "cfg4_pd784": ("config 4", 1024)}
MFMA_FP32_FLOPS = 157.3e12
HBM_BYTES_PER_S = 6.0e12


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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.configs.split(","):
        label, B = CONFIGS[name]
        plan = Plan.load(os.path.join(ROOT, "tests", "golden", name))
        hc = HipCircuit(plan, init_plan_tensors(plan), device=dev)
        D = plan.num_variables
        lower = list(range(D // 2, D))
        x = hc.sample(B, seed=2)
        hc.expected_statistics(x, lower)  # (binds the chunk sizes, builds every table)
        es = _expected(hc)
        ps, s = es.ps, es.ps.s
        xm = s.evidence_batch(x, lower)
        chunks = ps.down.chunks_of(B, None)
        bad = torch.zeros(B, dtype=torch.int32, device=dev)
        live = torch.ones(B, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        zc = s._z_circuit()
        edge, leaf, unit = es.accumulators()

        def each(fn):
            def run():
                for r0, nb in chunks:
                    fn(r0, nb, zc._bindings[nb])
            return run

        phases = {
            "evidence_forward_ms": lambda: [ps.evidence_forward(xm[r0 : r0 + nb], bad[r0:], stream) for r0, nb in chunks],
            "flow_pass_ms": each(lambda r0, nb, bd: ps.flow_pass(bd, stream)),
            "unit_sums_ms": each(lambda r0, nb, bd: es.unit_sums(bd, ps.down._buffers[nb][0], live[r0 : r0 + nb], unit, stream)),
            "edge_sums_ms": each(lambda r0, nb, bd: es.edge_sums(bd, ps.down._buffers[nb][0], live[r0 : r0 + nb], edge, stream)),
            "leaf_sums_ms": each(lambda r0, nb, bd: es.leaf_sums(bd, ps.down._buffers[nb][0], xm[r0 : r0 + nb], live[r0 : r0 + nb],
                                                                 leaf, stream)),
        }
        row = {"config": label, "plan": name, "B": B, "missing": len(lower), "chunks": len(chunks),
               "call_ms": round(_time(lambda: hc.expected_statistics(x, lower), args.reps, args.warmup), 4)}
        for k, fn in phases.items():
            row[k] = round(_time(fn, args.reps, args.warmup), 4)
        yard = row["evidence_forward_ms"] + row["flow_pass_ms"]
        stats = row["unit_sums_ms"] + row["edge_sums_ms"] + row["leaf_sums_ms"]
        flops = sum(2.0 * B * d["F"] * d["Ko"] * d["M"] for d in s.layers if d["kind"] in SUM_KINDS)
        arena_bytes = 2.0 * hc.arena_bytes(B)
        floor = max(flops / MFMA_FP32_FLOPS, arena_bytes / HBM_BYTES_PER_S) * 1e3
        row.update({"yardstick_ms": round(yard, 4), "statistics_over_yardstick": round(stats / yard, 3),
                    "edge_flops": flops, "arena_bytes": arena_bytes, "edge_floor_ms": round(floor, 4),
                    "edge_over_floor": round(row["edge_sums_ms"] / floor, 2)})
        print(json.dumps(row), flush=True)
        del xm, edge, leaf, unit
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
