#!/usr/bin/env python3
"""Autoregressive conditionals and coding of squared circuits (`HipSquaredCircuit.autoregressive_log_probs` /
`autoregressive_conditionals` / `coding_tables`, DESIGN.md section 11 "Autoregressive conditionals and coding of squared
circuits") on BASELINE config 5 (`cfg5_sos_c_k32`: 784 pixels, Embedding-256, K = 32, complex-lse-sum), all 784 steps of the
default order.

    python scripts/bench_squared_autoregressive.py [--reps 10] [--warmup 3] [--rows 256 8] [--skip-codec]

HIP events around each timed call after `--warmup` untimed ones, in one process; the median is reported, with the smallest and
the largest of the timed calls.  Per batch size one JSON line each:

(a) the three all-steps calls: one forward of c and one launch over (row, step) per chunk of rows;
(b) the composition they replace, timed the same way as ONE unit: 784 calls of `posterior(x, order[i], order[i + 1:])`, each a
    forward of c plus a path launch; the conditionals of the two are compared;
(c) with the codec: `compress` (tables from one all-steps call) and one stepwise `decompress` (784 one-step calls with a
    host round trip each) in wall time, and the coded, quantised-ideal and -log2 p(x) bits per dimension of the rows.

The rows are samples of the model itself (`sq.sample`, seed 7), so the bits per dimension are those of data the model fits.
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
from cirkit_amd.initializers import init_plan_tensors  # noqa: E402
from cirkit_amd.plan import Plan  # noqa: E402
from cirkit_amd.squared import HipSquaredCircuit  # noqa: E402


def _time(fn, reps: int, warmup: int) -> dict:
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
    return {"ms": round(float(np.median(ts)), 3), "min_ms": round(float(min(ts)), 3), "max_ms": round(float(max(ts)), 3)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 8])
    ap.add_argument("--skip-codec", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    golden = os.path.join(ROOT, "tests", "golden")
    plan = Plan.load(os.path.join(golden, "cfg5_sos_c_k32"))
    with np.load(os.path.join(golden, "cfg5_sos_c_k32_golden.npz")) as z:  # (the committed weights: signed, trained scale)
        tensors = {k[2:]: z[k] for k in z.files if k.startswith("w_")}
    if not tensors:
        tensors = init_plan_tensors(plan)
    D = plan.num_variables
    sq = HipSquaredCircuit(plan, tensors, device=dev)
    order = sq.graph.tree_order()
    later = []
    for i in range(D):
        m = torch.zeros(D, dtype=torch.bool)
        m[order[i + 1:]] = True
        later.append(m)
    for B in args.rows:
        x = sq.sample(B, seed=7)
        assert bool((x >= 0).all())
        res = {"plan": "cfg5_sos_c_k32", "B": B, "steps": D}
        res["autoregressive_log_probs"] = _time(lambda: sq.autoregressive_log_probs(x), args.reps, args.warmup)
        res["autoregressive_conditionals"] = _time(lambda: sq.autoregressive_conditionals(x), args.reps, args.warmup)
        res["mixed_launches"] = sq.last_mixed_launches
        res["coding_tables"] = _time(lambda: sq.coding_tables(x), args.reps, args.warmup)
        print(json.dumps(res), flush=True)

        def composed():
            return [sq.posterior(x, order[i], later[i]) for i in range(D)]

        t = _time(composed, args.reps, args.warmup)
        cond = sq.autoregressive_conditionals(x)
        ref = torch.stack(composed(), dim=1)
        fin = torch.isfinite(ref) & torch.isfinite(cond)
        line = {"plan": "cfg5_sos_c_k32", "B": B, "what": "784 calls of posterior", **t,
                "ratio_to_conditionals": round(t["ms"] / res["autoregressive_conditionals"]["ms"], 2),
                "ratio_to_log_probs": round(t["ms"] / res["autoregressive_log_probs"]["ms"], 2),
                "ratio_to_coding_tables": round(t["ms"] / res["coding_tables"]["ms"], 2),
                "max_abs_difference": float((ref - cond)[fin].abs().max()), "same_finite": bool((torch.isfinite(ref) == torch.isfinite(cond)).all())}
        del ref, cond
        print(json.dumps(line), flush=True)
        if args.skip_codec:
            continue
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        blobs, counts = codec.compress(sq, x, batched=True, return_counts=True)
        t_enc = time.perf_counter() - t0
        t0 = time.perf_counter()
        back = codec.decompress(sq, blobs)
        t_dec = time.perf_counter() - t0
        nll = -(sq.autoregressive_log_probs(x).double().sum(dim=1) / np.log(2.0)).cpu().numpy()
        joint = -(sq.log_prob(x).double() / np.log(2.0)).cpu().numpy()
        print(json.dumps({"plan": "cfg5_sos_c_k32", "B": B, "what": "codec", "precision": 16, "compress_batched_s": round(t_enc, 3),
                          "decompress_stepwise_s": round(t_dec, 3), "decompress_ms_per_step": round(1e3 * t_dec / D, 3),
                          "round_trip": bool(torch.equal(back, x.cpu())),
                          "coded_bpd": round(float(np.mean([8 * len(b) for b in blobs])) / D, 4),
                          "quantised_ideal_bpd": round(float(codec.ideal_bits(counts, 16).mean()) / D, 4),
                          "chain_rule_bpd": round(float(nll.mean()) / D, 4), "log_prob_bpd": round(float(joint.mean()) / D, 4)}), flush=True)


if __name__ == "__main__":
    main()
