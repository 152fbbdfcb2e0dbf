#!/usr/bin/env python3
"""Marginals of a squared circuit (`HipSquaredCircuit.log_marginal`, DESIGN.md section 11 "Marginals of squared circuits") on
BASELINE config 5 (`cfg5_sos_c_k32`: 784 pixels, Embedding-256, K = 32, complex-lse-sum), three masks -- the lower half of the
image, every second pixel, one pixel -- at 256 rows and at as many rows as one chunk holds (c's arena plus the mixed arena
within 2 GiB, capped by --max-rows).

    python scripts/bench_squared_marginal.py [--reps 10] [--warmup 3] [--rows-per-block 1,2,4] [--max-rows 4096]

HIP events around each timed call after `--warmup` untimed ones, in one process; the median is reported.  Per (mask, B, rows
per workgroup of the 32-unit launch): the number of mixed folds, the launches of `ck_squared_mixed_fwd`, ms per call of
`log_marginal`, and the time of c's forward alone (the same `HipCircuit`, the same batch, the same process).  Prints one JSON
line each.
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
    ap.add_argument("--rows-per-block", default="1")
    ap.add_argument("--max-rows", type=int, default=4096)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    golden = os.path.join(ROOT, "tests", "golden")
    plan = Plan.load(os.path.join(golden, "cfg5_sos_c_k32"))
    with np.load(os.path.join(golden, "cfg5_sos_c_k32_golden.npz")) as z:  # (the committed weights: signed, trained scale)
        tensors = {k[2:]: z[k] for k in z.files if k.startswith("w_")}
    if not tensors:
        tensors = init_plan_tensors(plan)
    D = plan.num_variables
    pix = np.arange(D)
    masks = {"lower_half": pix >= D // 2, "every_second_pixel": pix % 2 == 1, "one_pixel": pix == D // 2 + 14}
    for rpb in (int(v) for v in args.rows_per_block.split(",")):
        sq = HipSquaredCircuit(plan, tensors, device=dev, rows_per_block=rpb)
        for name, m in masks.items():
            mt = torch.from_numpy(m)
            mp = sq.classify(mt)
            chunk = min(sq.rows_per_chunk(mt), args.max_rows)
            for B in sorted({256, chunk}):
                x = torch.from_numpy(np.random.default_rng(4).integers(0, 256, size=(B, D))).to(dev)
                t_call = _time(lambda: sq.log_marginal(x, mt), args.reps, args.warmup)
                launches = sq.last_launches
                t_c = _time(lambda: sq.c(x), args.reps, args.warmup)
                t_lp = _time(lambda: sq.log_prob(x), args.reps, args.warmup)
                out = sq.log_marginal(x, mt)
                print(json.dumps({
                    "plan": "cfg5_sos_c_k32", "mask": name, "missing": int(m.sum()), "B": B, "rows_per_block": rpb,
                    "mixed_folds": mp.num_mixed, "launches": launches, "chunks": -(-B // sq.rows_per_chunk(mt)),
                    "call_ms": round(t_call, 4), "c_forward_ms": round(t_c, 4), "log_prob_ms": round(t_lp, 4),
                    "rows_per_s": round(B / (t_call * 1e-3)), "finite": bool(torch.isfinite(out).all()),
                }), flush=True)
                del x
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
