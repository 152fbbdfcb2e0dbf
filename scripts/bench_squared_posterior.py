#!/usr/bin/env python3
"""Posterior marginals of squared circuits (`HipSquaredCircuit.posterior_marginals`, DESIGN.md section 11 "Posterior marginals of
squared circuits") on BASELINE config 5 (`cfg5_sos_c_k32`: 784 pixels, Embedding-256, K = 32, complex-lse-sum) at 256 rows.

    python scripts/bench_squared_posterior.py [--reps 10] [--warmup 3] [--rows 256] [--skip-loop]

HIP events around each timed call after `--warmup` untimed ones, in one process; the median is reported.  One JSON line each:

(a) `posterior_marginals` with Q = the lower half of the image (392 pixels), the upper half observed: the whole call, its
    launch counts, and the same call split by events between its phases into c's forward, the mixed launches, the down launches
    and the leaf launch (summed over the chunks of rows);
(b) the same table the only way there was before: 392 calls of `posterior`, one per pixel with the other 391 integrated out,
    timed as one unit (the wall time of the first loop is printed on its own: it builds 392 host plans, and the sampler keeps
    eight); the two tables are compared;
(c) Q = one pixel through the new pass against one `posterior` call.
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

from cirkit_amd import squared_posterior as sp  # noqa: E402
from cirkit_amd.initializers import init_plan_tensors  # noqa: E402
from cirkit_amd.plan import Plan  # noqa: E402
from cirkit_amd.squared import HipSquaredCircuit  # noqa: E402

PHASES = ("c_forward", "mixed", "down", "leaf")


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


def _phases(sq, x, q, reps: int, warmup: int) -> dict:
    """Median over `reps` calls of the time between the events recorded after each phase, summed over the chunks of a call."""
    runs = []
    for i in range(warmup + reps):
        marks = []

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((name, e))

        mark("start")
        sp.query_log_marginals(sq, x, q, normalized=False, mark=mark)
        torch.cuda.synchronize()
        if i < warmup:
            continue
        tot = dict.fromkeys(PHASES, 0.0)
        for (_, e0), (name, e1) in zip(marks, marks[1:]):  # (a later chunk's c_forward starts at the leaf launch of the one before)
            tot[name] += e0.elapsed_time(e1)
        runs.append(tot)
    return {k + "_ms": round(float(np.median([r[k] for r in runs])), 4) for k in runs[0]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--skip-loop", action="store_true")
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
    lower = list(range(D // 2, D))
    t0 = time.perf_counter()
    sq.posterior_marginals(x, lower)
    torch.cuda.synchronize()
    first_call = time.perf_counter() - t0  # (with the host plan of the query and c's first forward)
    t_all = _time(lambda: sq.posterior_marginals(x, lower), args.reps, args.warmup)
    table = sq.posterior_marginals(x, lower)
    dp = sp.plan_of(sq, lower, None)
    line = {"plan": "cfg5_sos_c_k32", "what": "posterior_marginals", "B": B, "query_vars": len(lower), "states": C, "call_ms": round(t_all, 3),
            "mixed_launches": sq.last_mixed_launches, "down_launches": sq.last_down_launches, "down_folds": len(dp.down),
            "row_bytes": sp.row_bytes(sq, dp), "down_row_bytes": sp.down_row_values(sq, dp) * sq._esize, "rows_per_chunk": sp.chunk_rows(sq, dp),
            "first_call_s": round(first_call, 3), "finite": bool(torch.isfinite(table).all())}
    line.update(_phases(sq, x, lower, args.reps, args.warmup))
    print(json.dumps(line), flush=True)
    v = D // 2 + 14
    t_one_new = _time(lambda: sq.posterior_marginals(x, [v], [w for w in lower if w != v]), args.reps, args.warmup)
    new_launches = (sq.last_mixed_launches, sq.last_down_launches)
    t_one_old = _time(lambda: sq.posterior(x, v, [w for w in lower if w != v]), args.reps, args.warmup)
    one_new = sq.posterior_marginals(x, [v], [w for w in lower if w != v])[:, 0]
    one_old = sq.posterior(x, v, [w for w in lower if w != v])
    print(json.dumps({"plan": "cfg5_sos_c_k32", "what": "one pixel", "B": B, "var": v, "posterior_marginals_ms": round(t_one_new, 4),
                      "posterior_ms": round(t_one_old, 4), "mixed_launches": new_launches[0], "down_launches": new_launches[1],
                      "posterior_mixed_launches": sq.last_mixed_launches,
                      "max_abs_probability_difference": float((one_new.exp() - one_old.exp()).abs().max())}), flush=True)
    if args.skip_loop:
        return

    def loop():
        return torch.stack([sq.posterior(x, w, [u for u in lower if u != w]) for w in lower], dim=1)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    worst = float((loop().exp() - table.exp()).abs().max())
    first = time.perf_counter() - t0
    print(json.dumps({"plan": "cfg5_sos_c_k32", "what": "posterior per variable, first loop", "wall_s": round(first, 3),
                      "max_abs_probability_difference": worst}), flush=True)
    t_loop = _time(loop, args.reps, max(args.warmup - 1, 0))
    print(json.dumps({"plan": "cfg5_sos_c_k32", "what": "posterior per variable", "B": B, "calls": len(lower), "all_ms": round(t_loop, 2),
                      "call_ms": round(t_loop / len(lower), 4), "ratio_to_one_pass": round(t_loop / t_all, 1),
                      "max_abs_probability_difference": worst}), flush=True)


if __name__ == "__main__":
    main()
