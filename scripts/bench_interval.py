#!/usr/bin/env python3
"""Interval-evidence throughput (`HipCircuit.interval_log_prob`, DESIGN.md section 11 "Interval evidence") at BASELINE
config 2 (QuadTree-2, Categorical-256, K = 32; 4096 rows, every variable a range of 8 states) and config 4 (Poon-Domingos,
Gaussian, K = 64; 1024 rows, every variable its 8-bit bin [x - 1/512, x + 1/512]), following scripts/bench_posterior.py's
protocol.

    python scripts/bench_interval.py [--reps 20] [--warmup 5]

HIP events around each timed call after `--warmup` untimed ones; the median is reported.  Per config: the whole call, the
interval leaf launches alone (bound staging + one launch per input layer, replayed on the bindings the call left) and, for
scale, the point forward of the SAME layer-wise circuit on the same rows: both run the same inner launches, so the
difference is the leaf.  Prints one JSON line each.
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
from cirkit_amd.initializers import init_plan_tensors  # noqa: E402
from cirkit_amd.interval import _state  # noqa: E402
from cirkit_amd.plan import Plan  # noqa: E402
from cirkit_amd.sampling import chunk_rows  # noqa: E402

CONFIGS = {"cfg2_qt784": ("config 2", 4096), "cfg4_pd784": ("config 4", 1024)}


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
        x = hc.sample(B, seed=2)
        if x.is_floating_point():  # the 8-bit bin of every pixel
            lo, hi, what = x - 1 / 512, x + 1 / 512, "bins of width 1/256"
        else:  # 8 states around every pixel
            lo = (x - 4).clamp(0, 248)
            hi, what = lo + 7, "ranges of 8 states"
        y = hc.interval_log_prob(lo, hi)  # (binds the chunk sizes, builds the block sums)
        st = _state(hc)
        s = st.s
        zc = s._z_circuit()
        chunks = chunk_rows(B, None, hc.arena_bytes(1))
        blo, bhi = st.bounds(lo, hi, None)
        stream = torch.cuda.current_stream(dev).cuda_stream
        launches = []

        def leaves():
            launches.clear()
            for r0, nb in chunks:
                launches.append(st.leaves(zc._bindings[nb], blo[r0 : r0 + nb], bhi[r0 : r0 + nb], stream))

        def point_forward():
            for r0, nb in chunks:
                zc(x[r0 : r0 + nb])

        t_call = _time(lambda: hc.interval_log_prob(lo, hi), args.reps, args.warmup)
        t_leaf = _time(leaves, args.reps, args.warmup)
        t_point = _time(point_forward, args.reps, args.warmup)
        row = {"config": label, "plan": name, "B": B, "intervals": what, "chunks": len(chunks), "rows_per_chunk": chunks[0][1],
               "call_ms": round(t_call, 4), "interval_leaf_ms": round(t_leaf, 4), "leaf_launches": int(sum(launches)),
               "leaf_share_of_call": round(t_leaf / t_call, 3), "layerwise_point_forward_ms": round(t_point, 4),
               "finite_rows": int(torch.isfinite(y[:, 0, 0]).sum())}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
