#!/usr/bin/env python3
"""Leave-one-out throughput (`HipCircuit.conditional_log_probs`, `HipCircuit.leave_one_out`, DESIGN.md section 11
"Leave-one-out conditionals") at BASELINE config 2 (QuadTree-2, Categorical-256, K = 32; 4096 rows) and config 4
(Poon-Domingos, Gaussian, K = 64; 1024 rows), complete rows, following scripts/bench_posterior.py's protocol.

    python scripts/bench_leave_one_out.py [--reps 20] [--warmup 5] [--query 16]

HIP events around each timed call after `--warmup` untimed ones; the median is reported.  Per config: the whole
`conditional_log_probs` call, the whole `leave_one_out` call on the first `--query` variables, and the phases replayed one by
one on what the last call left -- the evidence forwards of every chunk (range check included), the derivative passes, the
(B, D) log-probability launches, the (B, Q, C) leaf launches -- next to `posterior_marginals`' flow pass on the same values.
The comparison is ONE `posterior_marginals` call with a single query variable, reported times D as the brute-force estimate
of all D conditionals.  Prints one JSON line per config.
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
from cirkit_amd.leave_one_out import _loo  # noqa: E402
from cirkit_amd.plan import Plan  # noqa: E402

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
    ap.add_argument("--query", type=int, default=16)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.configs.split(","):
        label, B = CONFIGS[name]
        plan = Plan.load(os.path.join(ROOT, "tests", "golden", name))
        hc = HipCircuit(plan, init_plan_tensors(plan), device=dev)
        D = plan.num_variables
        x = hc.sample(B, seed=2)
        query = list(range(args.query))
        lp = hc.conditional_log_probs(x)  # (binds the chunk sizes, builds every table)
        p = hc.leave_one_out(x, query)
        st = _loo(hc)
        ps, s = st.ps, st.ps.s
        gauss = st.check_query(query)
        q = st.query_tables(query, gauss)
        xm = s.evidence_batch(x, [])
        chunks = st.down.chunks_of(B, None)
        bad = torch.zeros(B, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        zc = s._z_circuit()

        def forwards():
            for r0, nb in chunks:
                ps.evidence_forward(xm[r0 : r0 + nb], bad[r0:], stream)

        def derivatives():
            for r0, nb in chunks:
                st.derivative_pass(zc._bindings[nb], stream)

        def flows():
            for r0, nb in chunks:
                ps.flow_pass(zc._bindings[nb], stream)

        def log_probs():
            for r0, nb in chunks:
                st.log_probs(zc._bindings[nb], st.down._buffers[nb][0], xm[r0 : r0 + nb], bad[r0:], lp[r0], stream)

        def leaves():
            for r0, nb in chunks:
                st.leaves(zc._bindings[nb], st.down._buffers[nb][0], q, gauss, bad[r0:], p[r0], stream)

        row = {"config": label, "plan": name, "B": B, "D": D, "query_vars": len(query), "states": int(p.shape[2]),
               "chunks": len(chunks), "rows_per_chunk": chunks[0][1], "bytes_per_row": st.down.bytes_per_row,
               "conditional_log_probs_ms": round(_time(lambda: hc.conditional_log_probs(x), args.reps, args.warmup), 4),
               "leave_one_out_ms": round(_time(lambda: hc.leave_one_out(x, query), args.reps, args.warmup), 4)}
        hc.conditional_log_probs(x)  # (the phases replay the values and derivatives of a complete-row call)
        row["evidence_forward_ms"] = round(_time(forwards, args.reps, args.warmup), 4)
        row["derivative_pass_ms"] = round(_time(derivatives, args.reps, args.warmup), 4)
        row["log_probs_ms"] = round(_time(log_probs, args.reps, args.warmup), 4)
        row["leaf_ms"] = round(_time(leaves, args.reps, args.warmup), 4)
        row["flow_pass_ms"] = round(_time(flows, args.reps, args.warmup), 4)
        one = _time(lambda: hc.posterior_marginals(x, [0]), args.reps, args.warmup)
        row["posterior_one_variable_ms"] = round(one, 4)
        row["brute_force_estimate_ms"] = round(one * D, 1)
        row["speedup_over_brute_force"] = round(one * D / row["conditional_log_probs_ms"], 1)
        print(json.dumps(row), flush=True)
        del p, lp, xm
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
