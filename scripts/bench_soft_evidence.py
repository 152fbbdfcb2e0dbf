#!/usr/bin/env python3
"""Soft-evidence throughput (`HipCircuit.soft_evidence_log_prob`, `HipCircuit.soft_posterior_marginals`, DESIGN.md
section 11 "Soft evidence") at BASELINE config 2 (QuadTree-2, Categorical-256, K = 32): 4096 rows, the lower half of the
image soft with the noisy-channel evidence log_lik = -(c - y)^2 / 8 around a sampled pixel y, the upper half observed;
following scripts/bench_interval.py's protocol.

    python scripts/bench_soft_evidence.py [--reps 20] [--warmup 5] [--rows 4096]

HIP events around each timed call after `--warmup` untimed ones; the median is reported.  Timed: both calls; the soft leaf
launches and the posterior leaf launches alone (replayed on the bindings and the flow arena the calls left), with the bytes
per second each achieves over the B S C 4 bytes of log_lik it must stream; and, for scale, `posterior_marginals(x, lower
half)` and the layer-wise point forward on the same rows.  Prints one JSON line.
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
from cirkit_amd.soft_evidence import _state  # noqa: E402


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
    ap.add_argument("--rows", type=int, default=4096)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    name, B = "cfg2_qt784", args.rows
    plan = Plan.load(os.path.join(ROOT, "tests", "golden", name))
    hc = HipCircuit(plan, init_plan_tensors(plan), device=dev)
    D = plan.num_variables
    soft = list(range(D // 2, D))  # the lower half of the 28 x 28 image
    x = hc.sample(B, seed=2)
    c = torch.arange(256, device=dev, dtype=torch.float32)
    ll = (-((c[None, None, :] - x[:, soft].to(torch.float32)[:, :, None]) ** 2) / 8.0).contiguous()
    lp = hc.soft_evidence_log_prob(ll, x, soft_vars=soft)
    p, lv = hc.soft_posterior_marginals(ll, x, soft_vars=soft, return_log_evidence=True)  # (binds the chunks, builds the tables)
    st, ids = _state(hc, ll, x, soft)
    s = st.s
    zc = s._z_circuit()
    chunks = st.down.chunks_of(B, None)
    q = st._sets.get(ids, False)
    stream = torch.cuda.current_stream(dev).cuda_stream
    bad = torch.zeros(B, dtype=torch.int32, device=dev)
    launches = []

    def soft_leaf():
        launches.clear()
        for r0, nb in chunks:
            launches.append(st.soft_leaf(zc._bindings[nb], q, ll[r0 : r0 + nb], bad[r0:], stream))

    def posterior_leaf():
        for r0, nb in chunks:
            st.posterior_leaf(zc._bindings[nb], st.down._buffers[nb][0], q, ll[r0 : r0 + nb], bad[r0:], p[r0], lv[r0:], stream)

    def point_forward():
        for r0, nb in chunks:
            zc(x[r0 : r0 + nb])

    t_lp = _time(lambda: hc.soft_evidence_log_prob(ll, x, soft_vars=soft), args.reps, args.warmup)
    t_post = _time(lambda: hc.soft_posterior_marginals(ll, x, soft_vars=soft), args.reps, args.warmup)
    t_leaf = _time(soft_leaf, args.reps, args.warmup)
    t_pleaf = _time(posterior_leaf, args.reps, args.warmup)
    t_pm = _time(lambda: hc.posterior_marginals(x, soft), args.reps, args.warmup)
    t_point = _time(point_forward, args.reps, args.warmup)
    nbytes = ll.numel() * 4
    row = {"config": "config 2", "plan": name, "B": B, "soft_vars": len(soft), "log_lik_bytes": nbytes, "chunks": len(chunks),
           "rows_per_chunk": chunks[0][1], "soft_evidence_log_prob_ms": round(t_lp, 4),
           "soft_posterior_marginals_ms": round(t_post, 4), "soft_leaf_ms": round(t_leaf, 4),
           "soft_leaf_launches": int(sum(launches)), "soft_leaf_GBps": round(nbytes / t_leaf / 1e6, 1),
           "posterior_leaf_ms": round(t_pleaf, 4), "posterior_leaf_GBps_read": round(nbytes / t_pleaf / 1e6, 1),
           "posterior_marginals_ms": round(t_pm, 4), "layerwise_point_forward_ms": round(t_point, 4),
           "finite_rows": int(torch.isfinite(lp[:, 0, 0]).sum()),
           "max_row_sum_error": float((p.sum(2) - 1).abs().max())}
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
