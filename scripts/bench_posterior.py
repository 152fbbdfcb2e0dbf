#!/usr/bin/env python3
"""Posterior-marginal throughput (`HipCircuit.posterior_marginals`, DESIGN.md section 11 "Posterior marginals") at BASELINE
config 2 (QuadTree-2, Categorical-256, K = 32) and config 4 (Poon-Domingos, Gaussian, K = 64), half-image evidence (the upper
392 pixels observed), following scripts/bench_sample_cond.py's protocol.

    python scripts/bench_posterior.py [--reps 20] [--warmup 5] [--sizes 4096,65536] [--small-query 16]

HIP events around each timed call after `--warmup` untimed ones; the median is reported.  Per (config, B): the whole call,
and its three phases replayed one by one on what the last call left -- the evidence forwards of every chunk (range check
included), the flow passes, the leaf launches.  At 4096 rows the query set is the lower half (392 variables: a 1.6 GB output at
config 2); at larger B the leaf and the call use the first `--small-query` variables of the lower half, so that the (B, Q, C)
output fits in memory, while the flow pass does not depend on the query set.  Comparison rows on the same evidence:
`sample_conditional`, `mpe`, and the brute-force route for ONE query variable (C + 1 marginal forwards `hc(x,
integrate_vars=...)`; discrete configs only).  Prints one JSON line each.
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
from cirkit_amd.plan import Plan  # noqa: E402
from cirkit_amd.posterior import _state, query_ids  # noqa: E402

CONFIGS = {"cfg2_qt784": "config 2", "cfg4_pd784": "config 4"}


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
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--small-query", type=int, default=16)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.configs.split(","):
        label = CONFIGS[name]
        plan = Plan.load(os.path.join(ROOT, "tests", "golden", name))
        hc = HipCircuit(plan, init_plan_tensors(plan), device=dev)
        D = plan.num_variables
        lower = list(range(D // 2, D))
        mask = torch.from_numpy(np.arange(D) >= D // 2).to(dev)
        for B in (int(v) for v in args.sizes.split(",")):
            x = hc.sample(B, seed=2)
            query = lower if B <= 4096 else lower[: args.small_query]
            p = hc.posterior_marginals(x, query)  # (binds the chunk sizes, builds every table)
            st = _state(hc)
            s = st.s
            gauss = st.check_query(query_ids(query, D))
            q = st.query_tables(query, gauss)
            xm = s.evidence_batch(x, lower)  # (the evidence of the phases: the whole lower half masked)
            chunks = st.down.chunks_of(B, None)
            bad = torch.zeros(B, dtype=torch.int32, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            zc = s._z_circuit()

            def forwards():
                for r0, nb in chunks:
                    st.evidence_forward(xm[r0 : r0 + nb], bad[r0:], stream)

            def flows():
                for r0, nb in chunks:
                    st.flow_pass(zc._bindings[nb], stream)

            def leaves():
                for r0, nb in chunks:
                    bd = zc._bindings[nb]
                    st.leaves(bd, st.down._buffers[nb][0], q, gauss, bad[r0:], p[r0], None, stream)

            t_call = _time(lambda: hc.posterior_marginals(x, query), args.reps, args.warmup)
            t_fwd = _time(forwards, args.reps, args.warmup)
            t_flow = _time(flows, args.reps, args.warmup)
            t_leaf = _time(leaves, args.reps, args.warmup)
            out_bytes = p.numel() * 4
            row = {"config": label, "plan": name, "B": B, "observed": D - D // 2, "query_vars": len(query),
                   "states": int(p.shape[2]), "output_bytes": out_bytes, "chunks": len(chunks), "rows_per_chunk": chunks[0][1],
                   "call_ms": round(t_call, 4), "evidence_forward_ms": round(t_fwd, 4), "flow_pass_ms": round(t_flow, 4),
                   "leaf_ms": round(t_leaf, 4), "leaf_output_GB_per_s": round(out_bytes / (t_leaf * 1e-3) / 1e9, 1),
                   "bytes_per_row": st.down.bytes_per_row}
            del p
            torch.cuda.empty_cache()
            row["sample_conditional_ms"] = round(_time(lambda: hc.sample_conditional(x, mask, seed=1), args.reps, args.warmup), 4)
            row["mpe_ms"] = round(_time(lambda: hc.mpe(x, mask), args.reps, args.warmup), 4)
            if not gauss:  # one query variable by brute force: C + 1 marginal forwards
                C = int(q["C"])
                v = lower[0]
                rest = [u for u in lower if u != v]
                xs = x.clone()

                def brute():
                    hc(x, integrate_vars=lower)
                    for c in range(C):
                        xs[:, v] = c
                        hc(xs, integrate_vars=rest)

                row["brute_force_one_variable_ms"] = round(_time(brute, max(3, args.reps // 4), 1), 4)
            print(json.dumps(row), flush=True)
            del xm
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
