#!/usr/bin/env python3
"""Sampling squared circuits (`HipSquaredCircuit.state_log_marginals` / `sample`, DESIGN.md section 11 "Sampling squared
circuits") on BASELINE config 5 (`cfg5_sos_c_k32`: 784 pixels, Embedding-256, K = 32, complex-lse-sum) at 256 rows.

    python scripts/bench_squared_sampling.py [--reps 10] [--warmup 3] [--rows 256] [--skip-sample]

HIP events around each timed call after `--warmup` untimed ones, in one process; the median is reported.  One JSON line each:

(a) one step: `state_log_marginals` of one pixel over all 256 states with the pixels after it (raster order) integrated out;
(b) the same (B, 256) table the way it was obtained before: 256 calls of `log_marginal`, one per state with ``x_v = s``, timed
    as one unit; the two tables are compared;
(c) a full 784-step `sample` in the default order: its launches of `ck_squared_mixed_fwd` (0), the wall time of the first
    call (building the plan of the order) and of later calls.
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

from cirkit_amd.initializers import init_plan_tensors  # noqa: E402
from cirkit_amd.plan import Plan  # noqa: E402
from cirkit_amd.squared import HipSquaredCircuit  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--skip-sample", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    golden = os.path.join(ROOT, "tests", "golden")
    plan = Plan.load(os.path.join(golden, "cfg5_sos_c_k32"))
    with np.load(os.path.join(golden, "cfg5_sos_c_k32_golden.npz")) as z:  # (the committed weights: signed, trained scale)
        tensors = {k[2:]: z[k] for k in z.files if k.startswith("w_")}
    if not tensors:
        tensors = init_plan_tensors(plan)
    D, B, C = plan.num_variables, args.rows, 256
    sq = HipSquaredCircuit(plan, tensors, device=dev)
    x = torch.from_numpy(np.random.default_rng(4).integers(0, C, size=(B, D))).to(dev)
    v = D // 2 + 14
    later = torch.from_numpy(np.arange(D) > v)
    t_step = _time(lambda: sq.state_log_marginals(x, v, later), args.reps, args.warmup)
    mixed = sq.last_mixed_launches
    table = sq.state_log_marginals(x, v, later)
    t_c = _time(lambda: sq.c(x), args.reps, args.warmup)
    print(json.dumps({"plan": "cfg5_sos_c_k32", "what": "state_log_marginals", "B": B, "states": C, "var": v, "missing": int(later.sum()),
                      "mixed_launches": mixed, "call_ms": round(t_step, 4), "c_forward_ms": round(t_c, 4),
                      "finite": bool(torch.isfinite(table).all())}), flush=True)
    xs = x.clone()

    def per_state():
        cols = []
        for st in range(C):
            xs[:, v] = st
            cols.append(sq.log_marginal(xs, later))
        return torch.stack(cols, dim=1)

    t_all = _time(per_state, args.reps, args.warmup)
    worst = float((per_state() - table).abs().max())
    print(json.dumps({"plan": "cfg5_sos_c_k32", "what": "log_marginal per state", "B": B, "calls": C,
                      "launches_per_call": sq.last_launches, "all_states_ms": round(t_all, 3), "call_ms": round(t_all / C, 4),
                      "ratio_to_one_step": round(t_all / t_step, 1), "max_abs_difference": worst}), flush=True)
    if args.skip_sample:
        return
    walls = []
    for i in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = sq.sample(B, seed=7 + i)
        t_host = time.perf_counter() - t0
        torch.cuda.synchronize()
        walls.append((t_host, time.perf_counter() - t0))
    print(json.dumps({"plan": "cfg5_sos_c_k32", "what": "sample", "B": B, "steps": D, "mixed_launches": sq.last_mixed_launches,
                      "path_launches": D, "first_call_host_s": round(walls[0][0], 3), "first_call_s": round(walls[0][1], 3),
                      "later_call_host_s": round(min(w[0] for w in walls[1:]), 3), "later_call_s": round(min(w[1] for w in walls[1:]), 3),
                      "ms_per_step": round(1e3 * min(w[1] for w in walls[1:]) / D, 4),
                      "valid": bool((out >= 0).all() and (out < C).all())}), flush=True)


if __name__ == "__main__":
    main()
