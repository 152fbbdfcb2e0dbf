#!/usr/bin/env python3
"""Leave-one-out conditionals of squared circuits (`HipSquaredCircuit.conditional_log_probs`, `leave_one_out`; DESIGN.md section 11
"Leave-one-out conditionals of squared circuits") on BASELINE config 5 (`cfg5_sos_c_k32`: 784 pixels, Embedding-256, K = 32,
complex-lse-sum) at 256 rows.

    python scripts/bench_squared_loo.py [--reps 10] [--warmup 3] [--rows 256] [--pixels 16]

The method of scripts/bench_squared_posterior.py: HIP events around each timed call after `--warmup` untimed ones, in one process;
the median is reported.  One JSON line each:

(a) `conditional_log_probs` and `leave_one_out` for all 784 pixels: the whole call, its launches, and the same call split by
    events between its phases into c's forward, the down launches and the leaf launch (summed over the chunks of rows);
(b) the down launches with the VALU form forced at K = 32 (`form` 1 of `ck_squared_loo_down`) next to the register-tile form;
(c) what there was before: `posterior(x, v, [])`, one call per pixel, for `--pixels` pixels spread over the image, compared with the
    columns of (a); its time for 784 pixels is SCALED from those calls, not measured.
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

from cirkit_amd import squared_loo as sl  # noqa: E402
from cirkit_amd.initializers import init_plan_tensors  # noqa: E402
from cirkit_amd.plan import Plan  # noqa: E402
from cirkit_amd.squared import HipSquaredCircuit  # noqa: E402

PHASES = ("c_forward", "down", "leaf")


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


def _phases(call, reps: int, warmup: int) -> dict:
    """Median over `reps` calls of the time between the events recorded after each phase, summed over the chunks of a call."""
    runs = []
    for i in range(warmup + reps):
        marks = []

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((name, e))

        mark("start")
        call(mark)
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
    ap.add_argument("--pixels", type=int, default=16)
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
    lp = sl.plan_of(sq, None)
    base = {"plan": "cfg5_sos_c_k32", "B": B, "query_vars": D, "states": C}
    for what, fn, with_mark in (
            ("conditional_log_probs", lambda: sq.conditional_log_probs(x), lambda m, f=0: sl.conditional_log_probs(sq, x, mark=m, form=f)),
            ("leave_one_out", lambda: sq.leave_one_out(x), lambda m, f=0: sl.leave_one_out(sq, x, mark=m, form=f))):
        t = _time(fn, args.reps, args.warmup)
        line = dict(base, what=what, call_ms=round(t, 3), loo_launches=sq.last_loo_launches, down_folds=len(lp.down),
                    row_bytes=sl.row_bytes(sq, lp), der_row_bytes=sl.der_row_values(sq, lp) * sq._esize,
                    rows_per_chunk=sq._chunk_rows(None, lambda: sl.row_bytes(sq, lp)), finite=bool(torch.isfinite(fn()).all()))
        line.update(_phases(with_mark, args.reps, args.warmup))
        print(json.dumps(line), flush=True)
        if what == "conditional_log_probs":
            valu = _phases(lambda m: with_mark(m, 1), args.reps, args.warmup)
            same = float((sl.conditional_log_probs(sq, x, form=1).exp() - fn().exp()).abs().max())
            print(json.dumps(dict(base, what="down launches, VALU form forced at K = 32", down_ms=valu["down_ms"], tile_form_down_ms=line["down_ms"],
                                  ratio=round(valu["down_ms"] / line["down_ms"], 2), max_abs_probability_difference=same)), flush=True)
    t_table = _time(lambda: sq.leave_one_out(x), args.reps, args.warmup)
    table = sq.leave_one_out(x)
    pixels = [int(v) for v in np.linspace(0, D - 1, args.pixels).round()]

    # pixel by pixel, each call timed in its steady state: the sampler keeps eight host plans, a loop over sixteen would rebuild them
    worst, t_loop = 0.0, 0.0
    for v in pixels:
        t_loop += _time(lambda: sq.posterior(x, v, []), args.reps, args.warmup)
        worst = max(worst, float((sq.posterior(x, v, []).exp() - table[:, v].exp()).abs().max()))
    scaled = t_loop / len(pixels) * D
    print(json.dumps(dict(base, what="posterior(x, v, []) per pixel", measured_pixels=len(pixels), measured_ms=round(t_loop, 2),
                          call_ms=round(t_loop / len(pixels), 4), scaled_to_all_pixels_ms=round(scaled, 1), scaled_not_measured=True,
                          ratio_to_leave_one_out=round(scaled / t_table, 1), mixed_launches_per_call=sq.last_mixed_launches,
                          max_abs_probability_difference=worst)), flush=True)


if __name__ == "__main__":
    main()
